"""The models of tests/mask_models.py on the host: every table decodes back
to the blob, every family still reaches the planner branch it is named for,
and every model is one a parity test can say something with (CPU only).

tests/test_gpu_mask_models.py runs the same models on every GRU_A kernel
form; a parity test on a saturated or silent model proves little, so the CPU
oracle alone must keep each of them alive over the three frames those tests
run: at most 10 % of the final GRU_A states beyond |s| = 0.99 and a mean
|pcm| above 100.  These are conditions on the models, not tolerances: a
family that misses gets other weights (mask_models.build's amplitude rule),
never another bound.  Measured with the oracle (stream 0, 3 frames):

    model                        GRU_A blocks  |s| > 0.99  mean |pcm|
    one_block                               2      0.0 %         518
    z_empty_r_long                       1104      0.5 %         596
    z_one_full                           1248      1.8 %         519
    h_only_long                           656      0.0 %         513
    units17_long                         1537      1.8 %         501
    units16_long                         1568      0.5 %         578
    at_caps                              3072      1.6 %         582
    same_bank                            2304      1.8 %         637
    same_bank_long                       1872      0.8 %         579
    dup_in_long                          1312      0.5 %         528
    cap_edges                            3112      1.8 %         594
    all17                                3216      2.6 %         598
    dense                               13824      0.5 %         561
    skewed_seed2 / 3 / 5                 1382      0.0 %     499-526
    one_block / z_one_full / dense fp32        0.0 / 2.1 / 0.3 %  518 / 519 / 572
    gru_b_every_second_block int8 / fp32       1.3 / 1.3 %        584 / 551
    gru_b_one_row_block_empty int8 / fp32      1.0 / 0.8 %        591 / 590

(the stock synthetic_model(1): 1.0 %, 591 int8; 0.8 %, 590 fp32).  The test
prints each model's figures before it asserts (pytest -s).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import lpcnet_amd as L
import mask_models as M
import oracle_lib as O
from test_model_tables import HOOKS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_FAMILIES = ("one_block", "z_one_full", "dense")
# every model the GPU tests run: (name, variant)
MODELS = ([(k, 0) for k in M.FAMILIES] + [(k, 1) for k in FP32_FAMILIES] +
          [("gru_b_" + kind, v) for kind in M.GRU_B_KINDS for v in (0, 1)])
IDS = ["%s-%s" % (n, "fp32" if v else "int8") for n, v in MODELS]

# family -> (the planner takes it, the plan is split, the wide split form exists)
PLAN = {
    "one_block": (1, 0, 0), "z_empty_r_long": (1, 1, 1), "z_one_full": (1, 1, 1), "h_only_long": (1, 1, 1),
    "units17_long": (1, 1, 0), "units16_long": (1, 1, 1), "at_caps": (1, 0, 0), "same_bank": (1, 0, 0),
    "same_bank_long": (1, 1, 1), "dup_in_long": (1, 1, 1), "cap_edges": (0, 0, 0), "all17": (0, 0, 0), "dense": (0, 0, 0),
    "skewed_seed2": (1, 1, 1), "skewed_seed3": (1, 1, 0), "skewed_seed5": (1, 1, 0),
}
CLASSES = ("1", "512", "1024", "2048", "8192/wide")


def blob_of(name, variant):
    if name.startswith("gru_b_"):
        return M.build_gru_b(name[len("gru_b_"):], variant)
    return M.model(name, variant)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """tools/model_host_check on every model's blob: its exit status, its
    output and {(model id, plan class, forced split): the fields of the
    plan's line}."""
    d = tmp_path_factory.mktemp("mask_models")
    paths = []
    for (name, variant), mid in zip(MODELS, IDS):
        p = d / mid
        p.write_bytes(blob_of(name, variant))
        paths.append(str(p))
    env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    subprocess.run(["make", "-C", ROOT, "tools/model_host_check"], check=True, capture_output=True, env=env)
    r = subprocess.run([os.path.join(ROOT, "tools", "model_host_check")] + paths, capture_output=True, text=True, env=env)
    table = {}
    for line in r.stdout.splitlines():
        m = re.match(r"plan (.*?): (.*)$", line)
        if not m:
            continue
        tag, rest = m.groups()
        forced = tag.endswith("/forced split")
        mid, cls = tag[len(str(d)) + 1:-len("/forced split")].split("/", 1) if forced else tag[len(str(d)) + 1:].split("/", 1)
        f = {}
        head, _, groups = rest.partition(" groups ")
        words = head.split()
        for key in ("variant", "may_saturate", "mf_ok", "fp_ok", "fp_long", "lockstep_streams", "split", "wide_split"):
            if key in words:
                f[key] = int(words[words.index(key) + 1])
        for key in ("own", "pieces"):
            if key in words:
                f[key] = [int(x) for x in words[words.index(key) + 1:words.index(key) + 4]]
        # per wave (own z/r, hosted z/r, own h, hosted h) groups
        f["groups"] = [tuple(int(x) for x in g.split()) for g in re.findall(r"\(([^)]*)\)", groups)]
        table[(mid, cls, forced)] = f
    return r, table


def test_every_table_decodes_to_its_blob(plans):
    """mf / mf_unit / mf_frow, the wide split tables and the GRU_B tiles of
    every model, every plan class, planned and forced to split, decode to the
    blob's matrices; the wide split form exists exactly where the mask allows."""
    r, table = plans
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1].startswith("model_host_check ok"), r.stdout[-500:]
    assert len(table) == len(MODELS) * len(CLASSES) * 2


@pytest.mark.parametrize("name,variant", MODELS, ids=IDS)
def test_engine_and_reference_parser_accept(name, variant):
    blob = blob_of(name, variant)
    L.validate_model(blob)
    if O.have_ref_parser():
        assert O.ref_parse(blob, variant)[0] == "accept"


@pytest.mark.parametrize("name,variant", MODELS, ids=IDS)
def test_not_saturating(plans, name, variant):
    """no int8 pair of the model can saturate maddubs (block_may_saturate):
    otherwise the matrix-core kernels are silently out of the picture"""
    f = plans[1][("%s-%s" % (name, "fp32" if variant else "int8"), "1", False)]
    assert f["variant"] == variant and f["may_saturate"] == 0


@pytest.mark.parametrize("name", sorted(PLAN))
def test_family_reaches_its_plan(plans, name):
    table = plans[1]
    mf_ok, split, wide = PLAN[name]
    assert wide == (split and M.wide_split_exists(M.FAMILIES[name]))
    for cls in CLASSES:
        f = table[(name + "-int8", cls, False)]
        assert f["mf_ok"] == mf_ok, cls
        if not mf_ok:
            assert not table[(name + "-int8", cls, True)]["mf_ok"]  # over-full stays over-full when forced
            continue
        assert f["split"] == split, cls
        assert f["wide_split"] == (wide if cls == "8192/wide" else 0), cls
        assert all((p > 0) == (max(len(r) for r in M.FAMILIES[name][48 * g:48 * g + 48]) > f["own"][g])
                   for g, p in enumerate(f["pieces"])), (cls, f)


def groups(plans, name, cls="1", forced=False):
    return plans[1][(name + "-int8", cls, forced)]["groups"]


def test_one_block_has_waves_without_groups(plans):
    for cls in CLASSES:
        g = groups(plans, "one_block", cls)
        assert sorted(g) == [(0, 0, 0, 0)] * 4 + [(0, 0, 1, 0), (1, 0, 0, 0)], cls
    # nothing to split off: the planner declines a forced split
    assert not plans[1][("one_block-int8", "1", True)]["mf_ok"]


def test_empty_z_gives_hosted_groups_without_own(plans):
    for cls in ("1", "512", "1024", "2048"):
        assert any(g[0] == 0 and g[1] == 3 for g in groups(plans, "z_empty_r_long", cls)), cls
    f = plans[1][("z_empty_r_long-int8", "1", False)]
    assert f["pieces"][0] == 0 and f["pieces"][1] == 16 and f["pieces"][2] == 0


def test_hosted_pieces_in_one_gate_only(plans):
    for name, gate in (("h_only_long", 2), ("same_bank_long", 2), ("z_one_full", 0), ("dup_in_long", 0), ("units17_long", 0)):
        f = plans[1][(name + "-int8", "1", False)]
        assert [p > 0 for p in f["pieces"]] == [g == gate for g in range(3)], name
        hosted = [(g[1], g[3]) for g in f["groups"]]
        assert any(h[0 if gate < 2 else 1] > 0 for h in hosted) and all(h[1 if gate < 2 else 0] == 0 for h in hosted), name
    f = plans[1][("units16_long-int8", "1", False)]
    assert f["pieces"][0] > 0 and f["pieces"][1] == 0 and f["pieces"][2] > 0


def test_rows_at_the_caps_fill_every_group(plans):
    for cls in CLASSES:
        assert groups(plans, "at_caps", cls) == [(4, 0, 8, 0)] * 6, cls
        assert groups(plans, "same_bank", cls) == [(3, 0, 6, 0)] * 6, cls
    # forced: z / r still whole, one hosted h group everywhere
    assert groups(plans, "at_caps", "1", True) == [(4, 0, 7, 1)] * 6


def test_skewed_seeds_have_own_zero_waves(plans):
    """the Sparsify-like masks leave waves whose own z/r or h count is 0
    beside hosted groups: the split dispatch's (0, F) forms"""
    for seed in M.SKEWED_SEEDS:
        g = groups(plans, "skewed_seed%d" % seed)
        assert any(x[0] == 0 and x[1] > 0 for x in g) or any(x[2] == 0 and x[3] > 0 for x in g), seed


@pytest.mark.parametrize("name,variant", MODELS, ids=IDS)
def test_oracle_keeps_the_model_alive(name, variant):
    """the conditions of the module docstring, on the CPU oracle alone"""
    o = O.Oracle(blob_of(name, variant), variant)
    f = L.synthetic_features(0, 3)[:, :20]
    pcm = np.stack([o.synthesize(f[i]) for i in range(3)])
    a, _ = o.state()
    sat = float(np.mean(np.abs(a) > 0.99))
    level = float(np.abs(pcm.astype(np.float64)).mean())
    print("%-28s |s| > 0.99: %.1f %%  mean |pcm| %.0f" % (name + ("-fp32" if variant else "-int8"), 100 * sat, level))
    assert sat <= 0.10
    assert level > 100
