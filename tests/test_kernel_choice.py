"""Which sample kernel and which frame path a batch, a launch and a call take
(host only).

Every sample kernel computes the same PCM bit for bit, so a wrong choice
shows only as a slower benchmark.  lpcnet_mi355x_kernel_choice answers for a
blob, a batch size, a CU count, a kernel mode, a custom rcpps table or not and
the current environment, without a device (include/lpcnet_mi355x.h gives the
layouts).  tests/golden/kernel_choice.json holds the answers of the commit
before the rules moved from engine.cpp into kernel_choice.cpp, produced by
that commit's own functions (profiles/r14/README.md): the move must not change
one of them.  A change that alters a rule on purpose regenerates the fixture
with

    python tests/test_kernel_choice.py tests/golden/kernel_choice.json

and says so.

Fixture layout: "cases" maps model/streams/mode/rcp/cus/env to [plan (13
ints), launch string, index into "calls"]; the launch string has two
characters per launch row, the kernel (0 lockstep, 1 mf, 2 mf2, 3 mfw, 4 fp;
'!' = the three dispatch chains of the old engine.cpp disagreed) and whether
its PCM store is coalesced ('-' on rows with preload / trace / stamps, where
the old batch-level expression was never asked); a "calls" string has one
character per call row, 'A' + the five path bits.
"""
import ctypes as C
import itertools
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_choice.json")
# (name, variant, saturating, skewed)
MODELS = [("int8", 0, False, False), ("int8_saturating", 0, True, False), ("int8_skewed", 0, False, True),
          ("fp32", 1, False, False), ("fp32_skewed", 1, False, True)]
# with 256 CUs the wide kernel starts above 1,024 streams, three groups at
# 3,072 and 9,216 and two at 2,048 and 4,096; 128 / 129 straddle
# OVERLAP_MAX_STREAMS, 2,047 / 2,048 MF2_MIN_STREAMS
STREAMS = [1, 128, 129, 512, 1024, 1025, 2047, 2048, 3072, 4096, 9216]
ENVS = ["-", "MF2=0", "MF2=1", "MFW=0", "MFW=1", "MF2=1,MFW=1", "MF2=0,MFW=1", "MFW=1,MFW_G=2", "MFW_G=3"]
CROSS_STREAMS = [1, 1024, 9216]
PATH_ENVS = ["NO_CHUNK=1", "NO_MULTIFRAME=1", "NO_OVERLAP=1", "LPC_EAGER=1", "NO_DIRECT_PCM=1"]
PATH_STREAMS = [1, 128, 129, 1024, 9216]
CHOICE_VARS = ["LPCNET_MF2", "LPCNET_MFW", "LPCNET_MFW_G", "LPCNET_NO_CHUNK", "LPCNET_NO_MULTIFRAME", "LPCNET_NO_OVERLAP",
               "LPCNET_LPC_EAGER", "LPCNET_NO_DIRECT_PCM"]
# planner and load hooks: none may leak in from the caller's environment
HOOKS = ["LPCNET_MF_ITERS", "LPCNET_MF_SIMD_W", "LPCNET_MF_HOSTED_F", "LPCNET_MF_PIECE_W", "LPCNET_MF_CAPS",
         "LPCNET_MF_FORCE_SPLIT", "LPCNET_NO_QUAD", "LPCNET_NO_MFMA", "LPCNET_NO_FPK", "LPCNET_FP_FORCE_LONG",
         "LPCNET_FC_EXACT", "LPCNET_MF_EXACT", "LPCNET_MF_ZR_BOUND", "LPCNET_NO_MFW_SPLIT", "LPCNET_RCP",
         "LPCNET_LPC_GAMMA", "LPCNET_FEATURES_DELAY", "LPCNET_END2END", "LPCNET_VERBOSE"] + CHOICE_VARS
PLAN = ["base", "mf2", "mfw", "mfw_g", "mfw_forced", "plan_wide", "rcp_hw", "quad_path", "streams_per_workgroup",
        "lds_bytes", "mfma_ops_per_group_sample", "plans_wide", "mf_ok"]
OVERLAP_MAX_STREAMS = 128


def case_keys():
    keys = []
    for m in MODELS:
        keys += [(m[0], s, 0, 0, 256, e) for s in STREAMS for e in ENVS]
        keys += [(m[0], s, mode, rcp, cus, "-") for s in CROSS_STREAMS for mode in (0, 1, 4, 5) for rcp in (0, 1)
                 for cus in (256, 128)]
        keys += [(m[0], s, 0, 0, 256, e) for s in PATH_STREAMS for e in PATH_ENVS]
    return list(dict.fromkeys(keys))


def key_name(k):
    return "/".join(str(x) for x in k)


def launch_rows(B, cus):
    """(nB, preload, trace, stamps)"""
    flags = [(0, 0, 0), (40, 0, 0), (0, 1, 0), (0, 0, 1)]
    return [(nB,) + f for nB in (1, 4 * cus, 4 * cus + 1, B) for f in flags]


def call_rows(B):
    """(nframes, N, nB, preload, chunking, has_fstream, trace, stamps, features_delay, end2end); a batch has its
    second queue up to OVERLAP_MAX_STREAMS streams"""
    fs = 1 if B <= OVERLAP_MAX_STREAMS else 0
    rows = [(nf, N, B, 0, ch, fs, tr, st, fd, e2e) for nf, N, ch, tr, st, fd, e2e in
            itertools.product((1, 2, 3, 4, 32), (0, 160), (1, 0), (0, 1), (0, 1), (0, 2), (0, 1))]
    # a teacher-forced call, a pool's narrow step of this batch, and the other answer about the second queue
    rows += [(1, 160, B, 40, 1, fs, 0, 0, 2, 0), (1, 160, 1, 0, 1, fs, 0, 0, 2, 0), (1, 160, OVERLAP_MAX_STREAMS + 1, 0, 1, fs, 0, 0, 2, 0),
             (2, 160, B, 0, 1, 1 - fs, 0, 0, 2, 0), (32, 160, B, 0, 0, 1 - fs, 0, 0, 2, 0)]
    return rows


def set_env(env, spec):
    for v in CHOICE_VARS:
        env.pop(v, None)
    if spec != "-":
        for kv in spec.split(","):
            name, val = kv.split("=")
            env["LPCNET_" + name] = val


def choice(L, blob, streams, cus, mode, rcp, launches, calls):
    """(plan, launch_out, call_out, the CU count planned for: cus, or with cus = 0 the current device's) of
    lpcnet_mi355x_kernel_choice under the current environment"""
    f = L.lib.lpcnet_mi355x_kernel_choice
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                  C.c_void_p, C.c_int, C.c_void_p]
    plan = (C.c_int * len(PLAN))()
    lin = (C.c_int * (4 * len(launches)))(*[x for r in launches for x in r])
    lout = (C.c_int * (2 * len(launches)))()
    cin = (C.c_int * (10 * len(calls)))(*[x for r in calls for x in r])
    cout = (C.c_int * (5 * len(calls)))()
    rc = f(blob, len(blob), streams, cus, mode, rcp, plan, lin, len(launches), lout, cin, len(calls), cout)
    assert rc > 0, L.last_error()
    return list(plan), list(lout), list(cout), rc


def encode(launches, lout, cout):
    ls = ""
    for i, (_, pre, tr, st) in enumerate(launches):
        k, co = lout[2 * i], lout[2 * i + 1]
        ls += ("!" if k < 0 else str(k)) + ("-" if pre or tr or st else str(co))
    cs = "".join(chr(65 + sum(cout[5 * i + j] << j for j in range(5))) for i in range(len(cout) // 5))
    return ls, cs


def all_choices(L, keys=None):
    for h in HOOKS:
        os.environ.pop(h, None)
    blobs = {m[0]: L.synthetic_model(1, m[1], saturating=m[2], skewed=m[3]) for m in MODELS}
    cases, calls = {}, []
    try:
        for k in keys or case_keys():
            model, streams, mode, rcp, cus, env = k
            set_env(os.environ, env)
            lr = launch_rows(streams, cus)
            plan, lout, cout, _ = choice(L, blobs[model], streams, cus, mode, rcp, lr, call_rows(streams))
            ls, cs = encode(lr, lout, cout)
            if cs not in calls:
                calls.append(cs)
            cases[key_name(k)] = [plan, ls, calls.index(cs)]
    finally:
        set_env(os.environ, "-")
    return {"cases": cases, "calls": calls}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    import lpcnet_amd as L
    saved = {h: os.environ.get(h) for h in HOOKS}
    try:
        return all_choices(L)
    finally:
        for h, v in saved.items():
            if v is None:
                os.environ.pop(h, None)
            else:
                os.environ[h] = v


def fixture_row(golden, model, streams, mode, rcp, cus, env):
    """a case's plan as a dict, or None when the fixture does not hold the case"""
    c = golden["cases"].get(key_name((model, streams, mode, rcp, cus, env)))
    return dict(zip(PLAN, c[0])) if c else None


def test_fixture_covers_the_matrix_and_every_branch(golden):
    cases = golden["cases"]
    assert set(cases) == {key_name(k) for k in case_keys()}
    plans = [dict(zip(PLAN, c[0])) for c in cases.values()]
    nlaunch, ncall = len(launch_rows(1, 256)), len(call_rows(1))
    assert all(len(c[0]) == len(PLAN) and len(c[1]) == 2 * nlaunch for c in cases.values())
    assert all(len(s) == ncall for s in golden["calls"])
    # the old engine's three dispatch chains agreed wherever more than one could run
    assert not any("!" in c[1] for c in cases.values())
    # each of the five kernels is launched somewhere, with both answers about its PCM store where it has two
    seen = {c[1][i:i + 2] for c in cases.values() for i in range(0, len(c[1]), 2)}
    assert {"0", "1", "2", "3", "4"} <= {s[0] for s in seen}
    assert {"00", "11", "10", "20", "31", "30", "41", "40"} <= seen
    assert {p["base"] for p in plans} == {0, 1, 4}
    # quad_path: the lockstep kernel without and with the quad layout, mf, fp, mf2, mfw
    assert {p["quad_path"] for p in plans} == {0, 1, 4, 5, 6, 7}
    assert {p["mfw_g"] for p in plans if p["mfw"]} == {2, 3}
    assert {p["mfw_forced"] for p in plans if p["mfw"]} == {0, 1}
    for f in ("mf2", "mfw", "plan_wide", "rcp_hw", "plans_wide", "mf_ok"):
        assert {p[f] for p in plans} == {0, 1}, f
    # mf2 without mfw, and the wide kernel's split form (the skewed model's: two groups)
    assert any(p["mf2"] and not p["mfw"] for p in plans)
    assert fixture_row(golden, "int8_skewed", 9216, 0, 0, 256, "-")["mfw_g"] == 2
    assert fixture_row(golden, "int8", 9216, 0, 0, 256, "-")["mfw_g"] == 3
    assert fixture_row(golden, "int8", 4096, 0, 0, 256, "-")["mfw_g"] == 2
    # both values of every path bit
    bits = {(j, (ord(ch) - 65) >> j & 1) for s in golden["calls"] for ch in s for j in range(5)}
    assert bits == {(j, v) for j in range(5) for v in (0, 1)}


@pytest.mark.parametrize("model", [m[0] for m in MODELS])
def test_choice_matches_the_parent(computed, golden, model):
    n = 0
    for name, want in golden["cases"].items():
        if name.split("/")[0] != model:
            continue
        got = computed["cases"][name]
        assert dict(zip(PLAN, got[0])) == dict(zip(PLAN, want[0])), name
        assert got[1] == want[1], name
        assert computed["calls"][got[2]] == golden["calls"][want[2]], name
        n += 1
    assert n == len(case_keys()) // len(MODELS)


def test_plan_class_follows_plans_wide(computed):
    """replan_if_needed compares plans_wide with the plan class the register tables were built for: after a load
    they agree for every model with such tables (no re-plan), and no other model has a plan class"""
    for name, (plan, _, _) in computed["cases"].items():
        p = dict(zip(PLAN, plan))
        assert p["plan_wide"] == (p["plans_wide"] if p["mf_ok"] else 0), name
        # the wide kernel only ever runs on tables planned for it
        assert not p["mfw"] or p["plan_wide"], name


if __name__ == "__main__":
    sys.path.insert(0, os.environ.get("LPCNET_TREE", os.path.dirname(HERE)))
    import lpcnet_amd
    with open(sys.argv[1], "w") as out:
        json.dump(all_choices(lpcnet_amd), out, indent=0, sort_keys=True)
        out.write("\n")
