"""The sampler role of the sample kernels -- the GRU_B update, the dual-FC tree
walk of sampler.h, the kiss99 thresholds and the signal tail of
lpcnet.c:235-271 -- on the cases of tests/sampler_cases.py, against
tests/golden/sampler_edge.npz and the live CPU oracle, on every kernel form.

A case is a 14-frame run of one stream (sampler_cases.SCHEDULE): plain frames,
a tail state written through save_state / restore_state after frame 3, a frame
with 77 and one with 160 teacher-forced samples, one of 81 samples and one of
1, then four frames in one device-resident lpcnet_batch_synthesize_frames
call.  Edge streams take the first streams of a batch (every position of the
first workgroups, both sides of their boundaries) and its last two (the
ragged end); lpcnet_mi355x_synthetic_features fills the rest, and oracle work
is done for the edge streams only, once per (model, case).

After every host frame and after the device run, for every edge stream: the
PCM against the fixture and the oracle; save_state against the oracle --
last_sig, deemph_mem, last_exc, the kiss99 words, both GRU states -- NaN
where the oracle is NaN (as cond_frames.canon), bit-equal elsewhere; where the
form traces (mf_kernel<1>, <4>, the lockstep kernel, fp_kernel), the eight
logits and the excitation of every sample.  A mismatch names model, case,
form, frame, field and first indices.

Forms (the kernel is asserted from info().kernel_name):
  mf1         mf_kernel<1, 0, false, true>     the edge streams alone
  mf2         mf_kernel<2, 0, false, true>     512 streams
  mf4         mf_kernel<4, 0, false, true>     1026 streams
  mf2_kernel  mf2_kernel<4, false, true>       9 streams (LPCNET_MF2=1)
  mfw2, mfw3  mfw_kernel<true, 2 / 3, false>   8 and 12 streams (LPCNET_MFW=1)
  fp          fp_kernel<0, ...>                fp32 models
  lockstep    sample_kernel<...>               int8, fp32 and the saturating model
  table       mf_kernel<1 / 4, 0, false, false> and fp_kernel<0, ..., false>: the
              host's rcpps table; every stream against the lockstep kernel
              with the same table (the oracle's table is process-global)
A launch with teacher-forced samples or tracing takes mf_kernel on the mf2 /
mfw batches (kernel_choice.cpp), so those runs also hand the sampler state
from one kernel to the other and back.

The walk form (select-free or exact tanh, MfTables::fc_fin) and the GRU_A
range bounds are read from the engine's LPCNET_VERBOSE lines: fc_mid and
fc_ramp must walk exactly, and ga_hbias's h conditioning must lie outside the
h bound.  ga_hbias and ga_zrbias put single GRU_A units out of range, one
lane of a wave at a time: their workgroups must take the exact elementwise
step (NaN states, INT_MIN seeds), which a range check that looks at lane 0
alone misses."""
import functools
import re

import numpy as np
import pytest

import lpcnet_amd as L
import sampler_cases as SC
from test_gpu_mask_models import setenv

pytestmark = pytest.mark.gpu

NFR, FRAME = SC.NFRAMES, SC.FRAME
D0, D1 = SC.DEVICE_FRAMES
TANH_FIN_BOUND = 2.0 ** 30  # device_math.h kTanhFinBound

# form -> (environment, set_kernel mode, streams (None: the edge streams alone), kernel name, traces)
FORMS = {
    "mf1": ({"LPCNET_MF2": "0"}, 4, None, "mf_kernel<1, 0, false, true>", True),
    "mf2": ({"LPCNET_MF2": "0"}, 4, 512, "mf_kernel<2, 0, false, true>", False),
    "mf4": ({"LPCNET_MF2": "0"}, 4, 1026, "mf_kernel<4, 0, false, true>", True),
    "mf2_kernel": ({"LPCNET_MF2": "1"}, 0, 9, "mf2_kernel<4, false, true>", False),
    "mfw2": ({"LPCNET_MF2": "1", "LPCNET_MFW": "1"}, 0, 8, "mfw_kernel<true, 2, false>", False),
    "mfw3": ({"LPCNET_MF2": "1", "LPCNET_MFW": "1", "LPCNET_MFW_G": "3"}, 0, 12, "mfw_kernel<true, 3, false>", False),
    "fp": ({}, 0, None, "fp_kernel<0, ", True),
    "fp_300": ({}, 0, 300, "fp_kernel<0, ", False),
    "lockstep": ({}, 1, None, "sample_kernel<", True),
}
INT8_FORMS = ["mf1", "mf2", "mf4", "mf2_kernel", "mfw2", "mfw3", "lockstep"]
FP32_FORMS = ["fp", "fp_300", "lockstep"]


def forms_of(key: str) -> list:
    var = key.rpartition("/")[2]
    return {"int8": INT8_FORMS, "fp32": FP32_FORMS, "sat": ["lockstep"]}[var]


@functools.lru_cache(maxsize=None)
def synthetic(B: int) -> np.ndarray:
    a = np.ascontiguousarray(np.stack([L.synthetic_features(s, NFR)[:, :SC.NF] for s in range(B)], 1))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle(key: str, case: str) -> dict:
    """the live oracle's run of a case, computed once and left unchanged"""
    r = SC.oracle_run(key, case)
    for v in r.values():
        v.setflags(write=False)
    return r


def layout(cases: list, B):
    """(B, [(stream, case)]): the cases in turn over the first streams of the
    batch -- at least 8, so every position of the first workgroups of 1, 2 and
    4 streams and of mf2 / mfw's 4-stream groups, and both sides of their
    boundaries -- and over its last two; a small batch is edge streams only."""
    n = len(cases)
    if B is None:
        B = max(n, 5)
    pos = list(range(B)) if B <= max(n, 12) else list(range(max(n, 8))) + [B - 2, B - 1]
    return B, [(p, cases[i % n]) for i, p in enumerate(pos)]


class Run:
    """One batch through the schedule: pcm [14, B, 160], the edge streams'
    save_state after every host frame and after the device run, every stream's
    after the device run, the trace of the host frames."""

    def __init__(self, key, edge, B, mode, trace=False, table=None):
        b = L.LPCNetBatch(B, 0, SC.model(key))
        b.set_kernel(mode)
        if table is not None:
            b.set_rcp_table(table)
        self.info = b.info()
        feats = synthetic(B).copy()
        teach = {f: np.tile(SC.teachers(key, edge[0][1])[f], (B, 1)) for f in (5, 7)}
        for p, c in edge:
            feats[:, p] = SC.features(key, c)
            for f in (5, 7):
                teach[f][p] = SC.teachers(key, c)[f]
        self.pcm = np.zeros((NFR, B, FRAME), np.int16)
        self.snaps, self.trace = {}, {}
        b.set_trace(trace)
        for f in range(D0):
            n, pre = SC.SCHEDULE[f]
            self.pcm[f, :, :n] = b.synthesize_impl(feats[f], teach[f], pre) if pre else b.synthesize(feats[f], n)
            if trace and f >= 2:  # the first two frames (FEATURES_DELAY) run no sample
                self.trace[f] = b.get_trace(n)
            if f == SC.TAIL_AFTER:
                for p, c in edge:
                    if c in SC.TAILS:
                        b.restore_state(p, SC.edit_snapshot(c, b.save_state(p)))
            for p, _ in edge:
                self.snaps[f, p] = b.save_state(p)
        b.set_trace(False)
        part = np.ascontiguousarray(feats[D0:D1])
        d_f, d_p = b.device_alloc(part.nbytes), b.device_alloc((D1 - D0) * B * FRAME * 2)
        b.h2d(d_f, part)
        b.synthesize_frames(None, d_f, d_p, D1 - D0)
        b.sync()
        b.d2h(self.pcm[D0:D1], d_p)
        b.device_free(d_f)
        b.device_free(d_p)
        self.final = [b.save_state(s) for s in range(B)]
        for p, _ in edge:
            self.snaps[D1 - 1, p] = self.final[p]
        b.close()


def words_diff(tag, f, name, got, exp) -> list:
    d = np.flatnonzero(got != exp)
    if not d.size:
        return []
    return ["%s frame %d: %s differs from the oracle's at %d indices, first %s: got %r, expected %r"
            % (tag, f, name, d.size, d[:6].tolist(), float(got[d[0]:d[0] + 1].view(np.float32)[0]),
               float(exp[d[0]:d[0] + 1].view(np.float32)[0]))]


def edge_errors(key, form, run: Run, edge) -> list:
    err = []
    for p, c in edge:
        tag = "%s %s on %s (stream %d of %d)" % (key, c, form, p, run.pcm.shape[1])
        o, fx = oracle(key, c), SC.expected(key, c)
        for f in range(NFR):
            for what, e in (("oracle's", o["pcm"][f]), ("fixture's", fx["pcm"][f])):
                d = np.flatnonzero(run.pcm[f, p] != e)
                if d.size:
                    err.append("%s frame %d: pcm differs from the %s at %d samples, first %s (got %d, expected %d)"
                               % (tag, f, what, d.size, d[:6].tolist(), run.pcm[f, p, d[0]], e[d[0]]))
            if (f, p) in run.snaps:
                tail, ga, gb = SC.snapshot_words(run.snaps[f, p])
                err += SC.tail_diff(tag, f, tail, o["tail"][f], "oracle's")
                err += SC.tail_diff(tag, f, tail, fx["tail"][f], "fixture's")
                err += words_diff(tag, f, "gru_a_state", ga, o["gru_a"][f])
                err += words_diff(tag, f, "gru_b_state", gb, o["gru_b"][f])
            if f in run.trace:
                n = SC.SCHEDULE[f][0]
                lg, ex = run.trace[f]
                err += words_diff(tag, f, "traced logits", SC.canon_floats(lg[p, :n]).ravel(), SC.canon_floats(o["logits"][f, :n]).ravel())
                d = np.flatnonzero(ex[p, :n] != o["exc"][f, :n])
                if d.size:
                    err.append("%s frame %d: traced excitation differs from the oracle's at samples %s" % (tag, f, d[:6].tolist()))
    return err


def report(err: list):
    assert not err, "%d mismatches; the first: %s" % (len(err), "\n".join(err[:8]))


WALK = re.compile(r"dual-FC walk: (\S+) form \(largest node bound (\S+),")
BOUNDS = re.compile(r"GRU_A range bounds: z/r (\S+) .*, h (\S+)")


def run_form(monkeypatch, capfd, key, form, cases):
    """The cases of a model on a form, in as many batches as they need:
    (mismatches, the engine's verbose lines)."""
    env, mode, B, kernel, traces = FORMS[form]
    setenv(monkeypatch, **env)
    for k in ("LPCNET_FC_EXACT", "LPCNET_MF_EXACT", "LPCNET_MF_ZR_BOUND", "LPCNET_MF_FORCE_SPLIT", "LPCNET_NO_MULTIFRAME", "LPCNET_RCP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LPCNET_VERBOSE", "1")
    capfd.readouterr()
    per = len(cases) if B is None or B > 12 else B
    err = []
    for i in range(0, len(cases), per):
        nB, edge = layout(cases[i:i + per], B)
        run = Run(key, edge, nB, mode, trace=traces)
        assert run.info.kernel_name.startswith(kernel), run.info.kernel_name
        err += edge_errors(key, form, run, edge)
    return err, capfd.readouterr().err


def check_walk_form(key: str, text: str):
    """the form the model's bound selects, as the engine reports it"""
    found = WALK.findall(text)
    assert found, "the engine did not report its walk form"
    want = "select-free" if SC.node_bound(key) < TANH_FIN_BOUND else "exact"
    for form, bound in found:
        assert form == want and float(bound) == pytest.approx(SC.node_bound(key), rel=1e-5), (form, bound, want)
    return want


# -- tail states -----------------------------------------------------------------------------------------

TAIL_PARAMS = [(m, f) for m in SC.PLAIN for f in forms_of(m)]


@pytest.mark.parametrize("key,form", TAIL_PARAMS, ids=["%s-%s" % p for p in TAIL_PARAMS])
def test_tail_states(require_gpu, monkeypatch, capfd, key, form):
    """Every tail state of sampler_cases.TAILS in one batch (two or three on
    the forms of 8, 9 and 12 streams) of a plain model."""
    err, text = run_form(monkeypatch, capfd, key, form, list(SC.TAILS))
    report(err)
    assert check_walk_form(key, text) == "select-free"


# -- edited models ---------------------------------------------------------------------------------------

MODEL_PARAMS = [("%s/%s" % (e, v), f) for e in SC.EDITED for v in SC.VARIANTS for f in forms_of(v)]


@pytest.mark.parametrize("key,form", MODEL_PARAMS, ids=["%s-%s" % p for p in MODEL_PARAMS])
def test_edited_models(require_gpu, monkeypatch, capfd, key, form):
    """An edited model's run on every edge position of a batch.  fc_mid and
    fc_ramp lie outside the select-free tanh's domain and must walk in the
    exact form; ga_hbias's h conditioning (1.2e9 and more) lies outside the
    GRU_A h bound and ga_zrbias's z / r conditioning outside the z/r bound,
    in single units, so their workgroups take the exact elementwise step."""
    err, text = run_form(monkeypatch, capfd, key, form, ["plain"])
    want = check_walk_form(key, text)
    name = key.partition("/")[0]
    assert (want == "exact") == (name in ("fc_mid", "fc_ramp")), (key, want)
    if name == "ga_hbias" and form.startswith("mf"):
        found = BOUNDS.findall(text)
        assert found, "the engine did not report its GRU_A range bounds"
        for _, h in found:
            assert 1.0 < float(h) < TANH_FIN_BOUND < min(abs(v) for v in SC.GA_HBIAS.values())
    if name == "ga_zrbias" and form.startswith("mf"):
        for zr, _ in BOUNDS.findall(text):
            assert 1000.0 < float(zr) < min(abs(v) for v in SC.GA_ZRBIAS.values())
    report(err)


# -- non-finite conditioning -----------------------------------------------------------------------------

COND_PARAMS = [(m, f) for m in SC.VARIANTS for f in forms_of(m)]


@pytest.mark.parametrize("key,form", COND_PARAMS, ids=["%s-%s" % p for p in COND_PARAMS])
def test_non_finite_conditioning_reaches_the_sample_kernels(require_gpu, monkeypatch, capfd, key, form):
    """cond_frames.NONFINITE plus loud and lpc_wide through synthesis: NaN and
    inf conditioning, a NaN GRU_A state, NaN LPC -- what the oracle computes,
    sample for sample and state for state."""
    err, _ = run_form(monkeypatch, capfd, key, form, ["cond:" + s for s in SC.NONFINITE])
    report(err)


# -- the table-only instances ---------------------------------------------------------------------------

def same_state(x: bytes, y: bytes) -> bool:
    """tail, GRU_A and GRU_B state of two save_state snapshots, NaN-canonical"""
    return all(np.array_equal(u, v) for u, v in zip(SC.snapshot_words(x), SC.snapshot_words(y)))


TABLE = [("int8", 4, None, "mf_kernel<1, 0, false, false>"), ("int8", 4, 1026, "mf_kernel<4, 0, false, false>"),
         ("fc_mid/int8", 4, None, "mf_kernel<1, 0, false, false>"), ("fp32", 0, None, "fp_kernel<0, ")]


@pytest.mark.parametrize("key,mode,B,kernel", TABLE, ids=["%s-%s" % (t[0], t[2] or "edge") for t in TABLE])
def test_table_only_instances_match_lockstep(require_gpu, monkeypatch, key, mode, B, kernel):
    """With the host's rcpps table the fast kernels run their table-only
    instances; the oracle's table is process-global, so every stream is held
    to the lockstep kernel with the same table: PCM of every frame, the edge
    streams' state after every frame and every stream's final state."""
    setenv(monkeypatch, LPCNET_MF2="0")
    table = L.host_rcp_table()[0]
    cases = ["plain"] if "/" in key else list(SC.TAILS)
    nB, edge = layout(cases, B)
    a = Run(key, edge, nB, mode, table=table)
    assert a.info.kernel_name.startswith(kernel) and a.info.rcp_hw == 0, a.info.kernel_name
    r = Run(key, edge, nB, 1, table=table)
    assert r.info.kernel_name.startswith("sample_kernel<"), r.info.kernel_name
    err = []
    d = np.argwhere(a.pcm != r.pcm)
    if d.size:
        err.append("%s: pcm differs from the lockstep kernel's in %d streams, first at frame %d stream %d sample %d"
                   % (key, len(set(d[:, 1].tolist())), d[0][0], d[0][1], d[0][2]))
    for k in a.snaps:
        if not same_state(a.snaps[k], r.snaps[k]):
            err.append("%s frame %d stream %d: the state differs from the lockstep kernel's" % ((key,) + k))
    bad = [s for s in range(nB) if not same_state(a.final[s], r.final[s])]
    if bad:
        err.append("%s: the final state of %d streams differs from the lockstep kernel's, first %s" % (key, len(bad), bad[:8]))
    report(err)
