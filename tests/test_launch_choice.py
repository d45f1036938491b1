"""Which kernel each launcher picks, pinned without a GPU.

Every kernel path is parity-exact, so a launch routed to a slower but correct
kernel passes the rest of the suite.  Here the launchers of csrc/ are compiled
host-only with tests/launch_recorder.hpp force-included (a launch becomes a text
record: instantiation, grid, block, LDS bytes, arguments), linked with
tests/launch_cases.hip and run over its table of cases.  The output -- one line
per distinct list of launches (instantiation, block, LDS bytes) with every
lookahead transition that occurs with it, and a count and hash of every line
of the full product (`launch_cases <family> --full` prints them) -- must equal
tests/golden/launch_choice_{nv,im,net}.txt line for line.  The goldens were
recorded from the launchers as they were before the launch choice was restated
(profiles/launch_paths/table.md); the InvMgmt one was recorded again when its
policy variants became template arguments, after its full product, with those
arguments deleted from the kernel names, had equalled the earlier one byte for
byte (profiles/im_variants/resources.md).
"""
import collections
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "or-gym-inventory_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
# common.hip is left out: the harness needs none of its launchers, and its
# kernels with external linkage would register a device binary that a
# host-only compile does not have
UNITS = ["newsvendor", "newsvendor_ph", "invmgmt", "invmgmt_ph", "invmgmt_rnd", "invmgmt_lvl", "invmgmt_ext",
         "netspec", "netinvmgmt"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the build's compiler) not found"
    out = tmp_path_factory.mktemp("launch_choice")
    flags = [hipcc, "--cuda-host-only", "-O0", "-std=c++17", "-I", CSRC, "-include", os.path.join(TESTS, "launch_recorder.hpp")]
    jobs = [(os.path.join(CSRC, u + ".hip"), str(out / (u + ".o"))) for u in UNITS]
    jobs.append((os.path.join(TESTS, "launch_cases.hip"), str(out / "launch_cases.o")))

    def compile_one(job):
        return subprocess.run(flags + ["-c", job[0], "-o", job[1]], capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=min(10, os.cpu_count() or 1)) as pool:
        for job, r in zip(jobs, pool.map(compile_one, jobs)):
            assert r.returncode == 0, f"{job[0]}:\n{r.stderr[-4000:]}"
    exe = str(out / "launch_cases")
    r = subprocess.run([hipcc, "-o", exe] + [o for _, o in jobs], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("family", ["nv", "im", "net"])
def test_launch_choice(harness, family):
    r = subprocess.run([harness, family], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    with open(os.path.join(TESTS, "golden", f"launch_choice_{family}.txt")) as f:
        want = f.read().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1} differs"
    assert len(got) == len(want)


# a launch record of an InvMgmt run or fused rollout kernel: name, template arguments, arguments
IM_POLICY_LAUNCH = re.compile(r" \| (im_run_kernel|im_roll3o?_kernel)<([^<>]*)> g=\d+ b=\d+ lds=\d+ \(([^()]*)\)")
# the trailing template arguments that name the policy variant (csrc/invmgmt.hip)
IM_VARIANT_ARGS = {"im_run_kernel": ("RND", "EXT", "LVL"), "im_roll3_kernel": ("RND", "LVL"),
                   "im_roll3o_kernel": ("RND", "LVL")}
# kernels.hpp POL_RANDOM, POL_EXTERNAL, POL_LEVELS; every other kind, and no policy (0): no variant
IM_VARIANT_OF_KIND = {6: "RND", 7: "EXT", 8: "LVL"}


def test_im_policy_variant_routing(harness):
    """Every InvMgmt run / rollout launch of the full product goes to the
    instantiation of its policy's variant: RANDOM to RND, EXTERNAL to EXT,
    LEVELS to LVL, every other kind and no policy to the one with none of the
    three.  The golden alone cannot say this: it names the instantiations that
    occur, not the policy each was launched for."""
    r = subprocess.run([harness, "im", "--full"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = collections.Counter()
    for line in r.stdout.splitlines():
        for name, targs, args in IM_POLICY_LAUNCH.findall(line):
            names = IM_VARIANT_ARGS[name]
            on = {n for n, v in zip(names, targs.split(", ")[-len(names):]) if v == "true"}
            kinds = [int(a[3:]) for a in args.split(",") if a.startswith("pol")]
            assert len(kinds) == 1, line
            want = IM_VARIANT_OF_KIND.get(kinds[0])
            assert on == ({want} if want else set()), line
            seen[(name, want)] += 1
    # the product reaches every instantiation family the rule speaks of
    for name, names in IM_VARIANT_ARGS.items():
        for want in (None,) + names:
            assert seen[(name, want)] > 0, (name, want)
