"""A float32 numpy restatement of the gradient kernels' head and backward pass
(csrc/ppo_grad.hip; TEST INFRASTRUCTURE, never shipped): 64-sample tiles, tile t
in workgroup t mod G, float32 sums inside a workgroup, the G partials added in
float64 and divided by n.  Not bit-exact (the matrix products are numpy's, not
the kernel's fmaf chains): it exists so that the CPU tests can hold the
kernel's arithmetic, and a list of plausible mistakes in it, against
tests/ppo_reference.py without a GPU.

``mistake``: one of MISTAKES, a deliberately wrong variant."""
import numpy as np

F32, F64 = np.float32, np.float64
TILE, MAX_GROUPS = 64, 256
LOGP0 = 0.91893853320467274178

MISTAKES = ("clip_side", "max_for_min", "clipped_grad", "no_minus_one", "no_entropy", "tanh_pre", "no_out_scale",
            "div_rows", "valid_ignored", "biased_std", "in_scale_row")


def _layers(module):
    """[(W [out, in], b [out])] float32 and whether a Tanh ends the module"""
    import torch
    mods = list(module)
    lin = [(m.weight.detach().numpy().astype(F32), m.bias.detach().numpy().astype(F32)) for m in mods
           if isinstance(m, torch.nn.Linear)]
    return lin, isinstance(mods[-1], torch.nn.Tanh)


def _act(v, kind):
    if kind == "relu":
        return np.where(v > 0, v, F32(0))
    return np.tanh(v.astype(F64)).astype(F32)


def _act_grad(d, y, pre, kind, mistake):
    if kind == "relu":
        return np.where(y > 0, d, F32(0))
    t = pre if mistake == "tanh_pre" else y
    return (d * (F32(1) - t * t)).astype(F32)


def _network_grads(case, net, head, mistake, idx):
    """the tiles, workgroups and the reduction around ``head(out, s, ok) -> (d loss / d out, extra
    per-sample rows or None, stat rows)``; returns (weight grads, bias grads, extra sums, stat sums, n)"""
    lin, out_tanh = _layers(case[net])
    scale = case["out_scale" if net == "actor" else "v_scale"]
    if mistake == "no_out_scale":
        scale_b = None
    else:
        scale_b = scale
    shift = case["out_shift" if net == "actor" else "v_shift"]
    rows_all = case["obs"] if case["obs0"] is None else np.concatenate([case["obs0"], case["obs"]])
    sel = np.arange(case["S"]) if idx is None else np.asarray(idx, np.int64)
    rows = len(sel)
    tiles = (rows + TILE - 1) // TILE
    G = min(tiles, MAX_GROUPS)
    pw = [np.zeros((G,) + w.shape, F32) for w, _ in lin]
    pb = [np.zeros((G,) + b.shape, F32) for _, b in lin]
    pe, ps = None, None
    for t in range(tiles):
        s = sel[t * TILE:(t + 1) * TILE]
        ok = np.ones(len(s), bool) if case["valid"] is None or mistake == "valid_ignored" else case["valid"][s]
        x = rows_all[s].astype(F32)
        if case["in_scale"] is not None:
            sc, sh = case["in_scale"].copy(), case["in_shift"].copy()
            if mistake == "in_scale_row":
                sc[0], sh[0] = 1, 0
            x = (x * sc + sh).astype(F32)
        x = np.where(ok[:, None], x, F32(0))            # a masked sample computes on zeros
        acts, pres, h = [x], [], x
        for l, (w, b) in enumerate(lin):
            pre = (h @ w.T + b).astype(F32)
            last = l == len(lin) - 1
            h = (_act(pre, "tanh") if out_tanh else pre) if last else _act(pre, case["act"])
            pres.append(pre)
            acts.append(h)
        out = h if scale is None else (h * scale + shift).astype(F32)
        with np.errstate(invalid="ignore", over="ignore"):
            d, extra, stat = head(out, s, ok)
        d = np.where(ok[:, None], d, F32(0)).astype(F32)
        if scale_b is not None:
            d = (d * scale_b).astype(F32)
        if out_tanh:
            d = _act_grad(d, acts[-1], pres[-1], "tanh", mistake)
        g = t % G
        if extra is not None:
            extra = np.where(ok[:, None], extra, F32(0)).astype(F32).sum(0, dtype=F32)
            pe = np.zeros((G,) + extra.shape, F32) if pe is None else pe
            pe[g] += extra
        stat = np.where(ok[:, None], stat, 0.0).sum(0)
        ps = np.zeros((G,) + stat.shape) if ps is None else ps
        ps[g] += stat
        for l in range(len(lin) - 1, -1, -1):
            pw[l][g] += (d.T @ acts[l]).astype(F32)
            pb[l][g] += d.sum(0, dtype=F32)
            if l:
                d = _act_grad((d @ lin[l][0]).astype(F32), acts[l], pres[l - 1], case["act"], mistake)
    n = ps[:, 0].sum()
    return [p.astype(F64).sum(0) for p in pw], [p.astype(F64).sum(0) for p in pb], \
        None if pe is None else pe.astype(F64).sum(0), ps.sum(0), n


def grads(case, mistake=None, idx="case"):
    """the structure of ppo_reference.grads, from float32 arithmetic in the kernels' grouping"""
    assert mistake is None or mistake in MISTAKES, mistake
    idx = case["idx"] if isinstance(idx, str) else idx
    A = case["A"]
    log_std = case["log_std"].astype(F32)
    std = np.exp(log_std.astype(F64)).astype(F32)
    clip = case["clip_range"]
    lo, hi = F32(1 - clip), F32(1 + clip)
    st = case["adv_stats"]

    def actor_head(mean, s, ok):
        z = ((case["raw"][s] - mean) / std).astype(F32)
        logp = (F32(-LOGP0 * A) - (F32(0.5) * z * z + log_std).sum(1, dtype=F32)).astype(F32)
        lr = (logp - case["old_logp"][s]).astype(F32)
        ratio = np.exp(lr).astype(F32)
        adv = case["adv"][s]
        if st is not None and st[0] >= 2:
            sd = np.sqrt(st[2] / (st[0] if mistake == "biased_std" else st[0] - 1.0)) + 1e-8
            adv = ((adv.astype(F64) - st[1]) / sd).astype(F32)
        s1, s2 = (adv * ratio).astype(F32), (adv * np.clip(ratio, lo, hi)).astype(F32)
        clipped = s2 < s1
        if mistake == "max_for_min":
            clipped = s2 > s1
        if mistake == "clip_side":
            clipped = ((adv > 0) & (ratio < lo)) | ((adv < 0) & (ratio > hi))
        chosen = np.where(clipped, s2, s1)
        g = np.where(clipped & (mistake != "clipped_grad"), F32(0), -s1).astype(F32)
        d = (g[:, None] * (z / std)).astype(F32)
        one = F32(0) if mistake == "no_minus_one" else F32(1)
        extra = (g[:, None] * (z * z - one)).astype(F32)
        stat = np.stack([np.ones(len(s)), -chosen.astype(F64), np.zeros(len(s)), ((ratio - F32(1)) - lr).astype(F64),
                         ((ratio < lo) | (ratio > hi)).astype(F64), ratio.astype(F64)], 1)
        return d, extra, stat

    def critic_head(v, s, ok):
        err = (v[:, 0] - case["returns"][s]).astype(F32)
        return (F32(2) * err)[:, None], None, np.stack([np.ones(len(s)), err.astype(F64) ** 2], 1)

    out = {}
    gw, gb, ge, ps, n = _network_grads(case, "actor", actor_head, mistake, idx)
    rows = case["S"] if idx is None else len(idx)
    div = rows if mistake == "div_rows" else n
    if n > 0:
        ent = 0.0 if mistake == "no_entropy" else case["ent_coef"]
        stats = np.array([n, ps[1] / div, float((0.5 + LOGP0 + log_std.astype(F64)).sum()), ps[3] / div, ps[4] / div,
                          ps[5] / div])
        out["actor"] = {"weight": [g / div for g in gw], "bias": [g / div for g in gb], "log_std": ge / div - ent,
                        "stats": stats}
    else:
        out["actor"] = {"weight": [g * 0 for g in gw], "bias": [g * 0 for g in gb], "log_std": ge * 0, "stats": np.zeros(6)}
    gw, gb, _, ps, n = _network_grads(case, "critic", critic_head, mistake, idx)
    div = rows if mistake == "div_rows" else n
    vf = case["vf_coef"]
    if n > 0:
        out["critic"] = {"weight": [g * vf / div for g in gw], "bias": [g * vf / div for g in gb],
                         "stats": np.array([n, ps[1] / div])}
    else:
        out["critic"] = {"weight": [g * 0 for g in gw], "bias": [g * 0 for g in gb], "stats": np.zeros(2)}
    for net in out:
        for k in ("weight", "bias"):
            out[net][k] = [np.asarray(g, F64).astype(F32).astype(F64) for g in out[net][k]]
    return out
