// The launch-choice harness of tests/test_launch_choice.py: calls the public
// launchers of csrc/ (compiled host-only with tests/launch_recorder.hpp
// force-included, so a launch is a text record) over a table of cases and
// prints one line per case:
//
//   <case> | <kernel instantiation> g=<grid> b=<block> lds=<bytes> (<arguments>) | ... -> ret=<hipError_t> la=<valid><slot> sunk=<0|1>
//
// A line holds every launch of the call in order (a commit launch first, the
// sub-launches of a split rollout each with their g0).  No HIP runtime function
// is called and no pointer is dereferenced: the device pointers are fake
// non-null values, ap_host is a real host array.
//
//   launch_cases nv|im|net          the reduced table (tests/golden/launch_choice_*.txt)
//   launch_cases nv|im|net --full   every case of the product
//
// (im prints a second table after the first, with a count and hash of its own:
// the specs at the ends of the range create accepts.)
//
// The product per family: stream x autoreset x t_u x K x io.obs x lookahead
// before the call x policy x (settings + shapes), where a setting is the
// default shape with one knob flipped, or a knob / N pair on either side of a
// count threshold, and a shape is a spec at the default knobs.
//
// The reduced table has one line per distinct list of launches (instantiation,
// block, LDS bytes; a sub-launch repeated over groups named once), followed by
// every lookahead transition that occurred with it in the full product:
//
//   <launches> :: <valid><slot>[c]><valid><slot>[s][!<hipError_t>] ...
//
// before > after the call; c = the cache was committed first (a *_commit_kernel
// launch in front), s = sunk, !n = the launcher returned error n.  It ends with
// the number of cases, of distinct (launches, transition) keys and an FNV-1a
// hash of all the full product's lines, so a change in any case of the product
// -- an argument, a grid, which case takes which path -- changes the reduced
// output.
#include "kernels.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace invsim;

namespace {

template <class T>
T *fake(uintptr_t v) {
    return reinterpret_cast<T *>(v);
}

constexpr int64_t N0 = 1000;
constexpr int EARLY_N = 32768;   // invmgmt.hip IM_EARLY_STORES_MIN_N
constexpr int AP_LDS = 256;      // invmgmt.hip IM_AP_LDS

struct Setting {
    std::string name;
    Knobs kn;
    int64_t N;
};
Setting setting(const char *name, int64_t n = N0) { return Setting{name, Knobs{}, n}; }

struct Out {
    bool full;
    // launches (instantiation, block, LDS bytes) -> the lookahead transitions seen with them
    std::map<std::string, std::set<std::string>> table;
    uint64_t hash = 1469598103934665603ull;
    long cases = 0;
    size_t keys = 0;
    void line(const std::string &desc, const std::string &rec, const Lookahead &before, hipError_t e,
              const Lookahead &after, int sunk) {
        char tail[64];
        snprintf(tail, sizeof tail, " -> ret=%d la=%d%d sunk=%d", (int)e, (int)after.valid, after.slot, sunk);
        const std::string l = desc + rec + tail;
        for (unsigned char c : l) hash = (hash ^ c) * 1099511628211ull;
        hash = (hash ^ '\n') * 1099511628211ull;
        cases++;
        if (full) {
            puts(l.c_str());
            return;
        }
        // the launches without grids and argument lists; a commit launch in
        // front is part of the transition ('c'), a repeated sub-launch is named once
        std::string sig, last;
        bool commit = false;
        for (size_t at = 0; (at = rec.find(" | ", at)) != std::string::npos;) {
            at += 3;
            const size_t g = rec.find(" g=", at), b = rec.find(" b=", at), arg = rec.find(" (", b);
            const std::string one = rec.substr(at, g - at) + rec.substr(b, arg - b);
            if (one.find("commit_kernel") != std::string::npos) commit = true;
            else if (one != last) sig += (sig.empty() ? "" : " | ") + one;
            last = one;
        }
        char tr[64];
        int n = snprintf(tr, sizeof tr, "%d%d%s>%d%d", (int)before.valid, before.slot, commit ? "c" : "", (int)after.valid,
                         after.slot);
        if (sunk) n += snprintf(tr + n, sizeof tr - n, "s");
        if (e != hipSuccess) snprintf(tr + n, sizeof tr - n, "!%d", (int)e);
        keys += table[sig].insert(tr).second;
    }
    void end() {
        if (full) return;
        for (const auto &row : table) {
            std::string l = row.first.empty() ? "(no launch)" : row.first;
            l += " ::";
            for (const std::string &t : row.second) l += " " + t;
            puts(l.c_str());
        }
        printf("# full product: %ld cases, %zu distinct keys, fnv1a64 %016llx\n", cases, keys, (unsigned long long)hash);
    }
};

struct Axes {   // the axes every family shares
    int philox, autoreset, ti, K, obs, la;
};
const char *AR[] = {"next", "same", "off"};
int t_of(int ti, int T) {
    const int v[5] = {-1, 0, T - 2, T - 1, T};
    return v[ti];
}
template <class F>
void for_axes(F f) {
    for (int ph = 0; ph < 2; ph++)
        for (int ar = 0; ar < 3; ar++)
            for (int ti = 0; ti < 5; ti++)
                for (int K : {1, 30})
                    for (int obs = 0; obs < 2; obs++)
                        for (int la = 0; la < 3; la++) f(Axes{ph, ar, ti, K, obs, la});
}
std::string axes_str(const Axes &a, int t_u) {
    char b[96];
    snprintf(b, sizeof b, "%s ar=%s t=%d K=%d obs=%d la=%d%d", a.philox ? "ph" : "np", AR[a.autoreset], t_u, a.K,
             a.obs, a.la > 0, a.la == 2);
    return b;
}
Lookahead la_of(const Axes &a) { return Lookahead{a.la > 0, a.la == 2 ? 1 : 0}; }
void fill_common(Common &cm, const Setting &st, const Axes &a) {
    cm.N = st.N;
    cm.Npad = pad_n(st.N);
    cm.autoreset = a.autoreset;
    cm.period = fake<int32_t>(0x100000);
    cm.status = fake<uint32_t>(0x110000);
    cm.philox = a.philox;
    cm.ph_step = 7;
    cm.kn = st.kn;
}
PolicyIO policy(int kind) {
    PolicyIO p{};
    p.kind = kind;
    p.mdim = 4;
    if (kind == POL_RANDOM) p.arng = fake<uint64_t>(0x200000);
    if (kind == POL_LEVELS || kind == POL_NET_LEVELS) p.levels = fake<const double>(0x210000);
    p.metrics = fake<double>(0x220000);
    return p;
}
template <class A, class O>
StepIO<A, O> step_io(const Axes &a) {
    StepIO<A, O> io{};
    io.K = a.K;
    io.act = fake<const A>(0x300000);
    io.obs = a.obs ? fake<O>(0x310000) : nullptr;
    io.rew = fake<double>(0x320000);
    io.term = fake<uint8_t>(0x330000);
    io.trunc = fake<uint8_t>(0x340000);
    return io;
}

// ------------------------------------------------------------------ Newsvendor
void run_nv(Out &out) {
    std::vector<Setting> sets = {setting("-"), setting("N0", 0)};
    auto flip = [&](const char *n, bool Knobs::*f) {
        Setting s = setting(n);
        s.kn.*f = !(s.kn.*f);
        sets.push_back(s);
    };
    flip("nv_roll", &Knobs::nv_roll);
    flip("nv_pol_roll", &Knobs::nv_pol_roll);
    flip("nv_ahead", &Knobs::nv_ahead);
    const int pols[] = {POL_NONE, POL_CONSTANT, POL_BASE_STOCK, POL_ORDER_UP_TO, POL_CLASSIC_NV, POL_SS, POL_RANDOM,
                        POL_EXTERNAL};
    const int T = 40;
    auto one = [&](const Setting &st, int L) {
        for_axes([&](const Axes &a) {
            for (int kind : pols) {
                NvParams p{};
                fill_common(p.cm, st, a);
                p.L = L;
                p.step_limit = T;
                p.pipe = fake<float>(0x400000);
                p.ahead = fake<uint64_t>(0x410000);
                p.pcon = fake<double>(0x420000);
                const int t_u = t_of(a.ti, T);
                const PolicyIO pol = policy(kind);
                const auto io = step_io<float, float>(a);
                const Lookahead la0 = la_of(a);
                Lookahead la = la0;
                launch_rec::buf().clear();
                const hipError_t e = nv_run_launch(p, t_u, kind ? &pol : nullptr, io, la, nullptr);
                char d[64];
                snprintf(d, sizeof d, "nv %s L=%d pol=%d ", st.name.c_str(), L, kind);
                out.line(d + axes_str(a, t_u), launch_rec::buf(), la0, e, la, 0);
            }
        });
    };
    for (const Setting &st : sets) one(st, 5);
    for (int L : {0, 1, 11, 16}) one(setting("-"), L);
}

// --------------------------------------------------------------------- InvMgmt
struct ImShape {
    std::string name;
    int M1, backlog, dist, lt_max, periods;
    int L[IM_MAX_M1];
};
void run_im(Out &out, bool limits) {
    std::vector<Setting> sets = {setting("-"), setting("N0", 0)};
    auto flip = [&](const char *n, bool Knobs::*f) {
        Setting s = setting(n);
        s.kn.*f = !(s.kn.*f);
        sets.push_back(s);
    };
    flip("im_split", &Knobs::im_split);
    flip("im_roll", &Knobs::im_roll);
    flip("im_pol_roll", &Knobs::im_pol_roll);
    flip("im_ahead", &Knobs::im_ahead);
    for (int g2 : {0, 1})
        for (int64_t n : {(int64_t)1000, (int64_t)960}) {   // 16 / 15 groups of 64 envs: even / odd
            Setting s = setting(g2 ? "im_roll3o_g2=1" : "im_roll3o_g2=0", n);
            s.kn.im_roll3o_g2 = (int8_t)g2;
            s.name += n == 1000 ? ",even" : ",odd";
            sets.push_back(s);
        }
    sets.push_back(setting("groups_odd", 960));
    for (int64_t m : {(int64_t)999, (int64_t)1000}) {
        Setting s = setting(m == 999 ? "im_roll3o_max_n=N-1" : "im_roll3o_max_n=N");
        s.kn.im_roll3o_max_n = m;
        sets.push_back(s);
        for (int64_t sub : {(int64_t)0, (int64_t)63, (int64_t)64, (int64_t)448, (int64_t)1024}) {   // 2-role rollout: sub-launches
            Setting u = s;
            u.kn.im_roll3o_max_n = 0;
            u.kn.im_roll_sub = sub;
            u.name = "im_roll3o_max_n=0,im_roll_sub=" + std::to_string(sub);
            if (sub == 63 || sub == 64) u.N = 200, u.name += ",N=200";   // one group per sub-launch: keep the line short
            if (m == 999) sets.push_back(u);
        }
    }
    sets.push_back(setting("N=early_min", EARLY_N));
    sets.push_back(setting("N=early_min+1", EARLY_N + 1));

    std::vector<ImShape> shapes;
    for (int backlog = 0; backlog < 2; backlog++)
        for (int dist : {1, 3, 5}) {
            auto add = [&](const char *n, int M1, int lt_max, int periods, std::initializer_list<int> L) {
                ImShape s{n, M1, backlog, dist, lt_max, periods, {}};
                int i = 0;
                for (int l : L) s.L[i++] = l;
                shapes.push_back(s);
            };
            add("m1", 1, 3, 30, {3});
            add("m3", 3, 10, 30, {1, 5, 10});
            add("m3other", 3, 10, 30, {2, 5, 10});
            add("m3lt16", 3, 16, 30, {1, 5, 16});
            add("m3long", 3, 10, AP_LDS + 1, {1, 5, 10});
            add("m3ap", 3, 10, AP_LDS, {1, 5, 10});
            add("m8", 8, 4, 30, {1, 2, 3, 4, 1, 2, 3, 4});
        }
    // the specs of tests/limit_cases.py at the ends of what create accepts (a
    // table of their own, after the first: its lines record their kernels and
    // LDS bytes); above_64k also past the EARLY threshold
    std::vector<ImShape> lim;
    for (int backlog = 0; backlog < 2; backlog++) {
        auto add = [&](const char *n, int lt_max, int periods, std::initializer_list<int> L) {
            ImShape s{n, (int)L.size(), backlog, 1, lt_max, periods, {}};
            int i = 0;
            for (int l : L) s.L[i++] = l;
            lim.push_back(s);
        };
        add("L255", 255, 300, {255});
        add("all_zero", 0, 9, {0, 0, 0, 0, 0, 0, 0, 0});
        add("od_max_4", 102, 120, {17, 102, 0});
        add("od_max_6", 61, 70, {61, 0, 1, 60, 5});
        add("od_max_9", 37, 45, {37, 0, 1, 36, 5, 37, 2, 9});
        add("above_64k", 40, 50, {17, 40, 3});
    }
    const int pols[] = {POL_NONE, POL_CONSTANT, POL_BASE_STOCK, POL_SS, POL_RANDOM, POL_EXTERNAL, POL_LEVELS};
    int max_periods = 0;   // ap_host is read at t_u <= periods
    for (const ImShape &sh : shapes) max_periods = std::max(max_periods, sh.periods);
    for (const ImShape &sh : lim) max_periods = std::max(max_periods, sh.periods);
    std::vector<double> ap(max_periods + 2);
    for (size_t i = 0; i < ap.size(); i++) ap[i] = 1.0 / (double)(i + 1);
    auto one = [&](const Setting &st, const ImShape &sh) {
        for_axes([&](const Axes &a) {
            for (int kind : pols) {
                ImParams p{};
                fill_common(p.cm, st, a);
                p.periods = sh.periods;
                p.lt_max = sh.lt_max;
                p.dist = sh.dist;
                int off = 0;
                for (int i = 0; i < sh.M1; i++) {
                    p.L[i] = sh.L[i];
                    p.ring_off[i] = off;
                    off += sh.L[i];
                }
                p.I = fake<int64_t>(0x500000);
                p.B = fake<int64_t>(0x510000);
                p.Rring = fake<int64_t>(0x520000);
                p.alog32 = fake<uint32_t>(0x530000);
                p.alog = fake<int64_t>(0x540000);
                p.ahead = fake<uint64_t>(0x1000000);
                const int t_u = t_of(a.ti, sh.periods);
                const PolicyIO pol = policy(kind);
                const auto io = step_io<int64_t, int64_t>(a);
                const Lookahead la0 = la_of(a);
                Lookahead la = la0;
                bool sunk = false;
                launch_rec::buf().clear();
                const hipError_t e =
                    im_run_launch(p, ap.data(), sh.M1, sh.backlog != 0, t_u, kind ? &pol : nullptr, io, la, sunk, nullptr);
                char d[128];
                snprintf(d, sizeof d, "im %s %s bl=%d dist=%d pol=%d ", st.name.c_str(), sh.name.c_str(), sh.backlog,
                         sh.dist, kind);
                out.line(d + axes_str(a, t_u), launch_rec::buf(), la0, e, la, sunk);
            }
        });
    };
    if (limits) {
        for (const ImShape &sh : lim) one(setting("-"), sh);
        for (const ImShape &sh : lim)
            if (sh.name == "above_64k") one(setting("N=early_min+1", EARLY_N + 1), sh);
        return;
    }
    for (const Setting &st : sets)
        for (const ImShape &sh : shapes)
            if (sh.name == "m3" && sh.dist == 1) one(st, sh);   // the settings: the default shape, both backlog modes
    for (const ImShape &sh : shapes)
        if (!(sh.name == "m3" && sh.dist == 1)) one(setting("-"), sh);
}

// ------------------------------------------------------------------ NetInvMgmt
void run_net(Out &out) {
    std::vector<Setting> sets = {setting("-"), setting("N0", 0)};
    auto flip = [&](const char *n, bool Knobs::*f) {
        Setting s = setting(n);
        s.kn.*f = !(s.kn.*f);
        sets.push_back(s);
    };
    flip("net_roll", &Knobs::net_roll);
    flip("net_roll3", &Knobs::net_roll3);
    flip("net_split", &Knobs::net_split);
    flip("net_pol_roll", &Knobs::net_pol_roll);
    flip("net_ahead", &Knobs::net_ahead);
    for (int64_t m : {(int64_t)999, (int64_t)1000, (int64_t)0}) {
        Setting s = setting("net_roll4_max_n");
        s.kn.net_roll4_max_n = m;
        s.name += "=" + std::to_string(m);
        sets.push_back(s);
    }
    struct Graph {
        const char *name;
        int which, J, E, RL, sumL, T;
    };
    const Graph graphs[] = {{"default", NET_SPEC_DEFAULT, 6, 11, 1, 61, 30},
                            {"custom", NET_SPEC_CUSTOM, 5, 5, 3, 4, 30},
                            {"defaultT257", NET_SPEC_DEFAULT, 6, 11, 1, 61, 257},   // past the rollout's alpha**t LDS table
                            {"generic", NET_SPEC_NONE, 4, 3, 2, 5, 30},
                            {"generic_big", NET_SPEC_NONE, 60, 120, 8, 100, 30},    // past the LDS limit
                            {"nospec", 3, 6, 11, 1, 61, 30}};                       // net_spec_launch refuses it
    const int pols[] = {POL_NONE, POL_CONSTANT, POL_BASE_STOCK, POL_RANDOM, POL_EXTERNAL, POL_NET_LEVELS};
    auto one = [&](const Setting &st, const Graph &g) {
        for (int rec = 0; rec < 2; rec++)
            for (int dem = 0; dem < 2; dem++)
                for (int nolevels = 0; nolevels < 2; nolevels++)
                    for_axes([&](const Axes &a) {
                        for (int kind : pols) {
                            if (nolevels && kind != POL_NET_LEVELS) continue;
                            NetParams p{};
                            fill_common(p.cm, st, a);
                            p.cm.info_rec = rec ? fake<void>(0x600000) : nullptr;
                            p.cm.info_demand = dem ? fake<int64_t>(0x610000) : nullptr;
                            p.J = g.J, p.E = g.E, p.RL = g.RL, p.sumL = g.sumL, p.T = g.T, p.backlog = 1;
                            p.X = fake<double>(0x620000);
                            p.ahead = g.which ? fake<uint64_t>(0x630000) : nullptr;
                            const int t_u = t_of(a.ti, g.T);
                            PolicyIO pol = policy(kind);
                            if (nolevels) pol.levels = nullptr;
                            const auto io = step_io<float, float>(a);
                            const Lookahead la0 = la_of(a);
                            Lookahead la = la0;
                            launch_rec::buf().clear();
                            const hipError_t e = g.which ? net_spec_launch(g.which, p, t_u, kind ? &pol : nullptr, io, la, nullptr)
                                                         : net_run_launch(p, t_u, kind ? &pol : nullptr, io, nullptr);
                            char d[128];
                            snprintf(d, sizeof d, "net %s %s rec=%d dem=%d pol=%d%s ", st.name.c_str(), g.name, rec, dem,
                                     kind, nolevels ? "(no levels)" : "");
                            out.line(d + axes_str(a, t_u), launch_rec::buf(), la0, e, la, 0);
                        }
                    });
    };
    for (const Setting &st : sets) one(st, graphs[0]);
    for (size_t i = 1; i < sizeof graphs / sizeof *graphs; i++) one(setting("-"), graphs[i]);
    one(setting("N0", 0), graphs[3]);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    Out out{argc > 2 && !strcmp(argv[2], "--full")};
    if (!strcmp(argv[1], "nv")) run_nv(out);
    else if (!strcmp(argv[1], "im")) {
        run_im(out, false);
        out.end();
        if (!out.full) puts("# the limit specs");
        Out lim{out.full};
        run_im(lim, true);
        lim.end();
        return 0;
    }
    else if (!strcmp(argv[1], "net")) run_net(out);
    else return 2;
    out.end();
    return 0;
}
