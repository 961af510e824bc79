"""The conditioning network on the device (run_frame_network, lpcnet.c:82-120:
frame_kernel.hip's FMA chains and chunk_kernel.hip's matrix-core tiles) on the
edge-case feature frames of tests/cond_frames.py, against
tests/golden/cond_edge.npz and the live CPU oracle.

Edge sequences occupy some streams of a batch -- the first, the last and both
sides of a workgroup boundary of the form under test --
lpcnet_mi355x_synthetic_features fills the rest, and oracle work is done for
the edge streams only.

* frame_kernel<1> (batches up to 256 streams: a stream per workgroup) and
  frame_kernel<4> (261 streams, chunking off): single-frame calls; after every
  frame the record of every edge stream (gru_a_cond, gru_b_cond, lpc, both
  conv memories, frame_count) on uint32 views against the fixture and the
  oracle, get_state against the oracle's frame(), the PCM against the
  oracle; every model of cond_frames.MODELS.
* the non-finite class through frame_only (N = 0) on both per-frame forms,
  and on chunk_kernel through lpcnet_batch_synthesize_frames with N = 0:
  above 128 streams that call takes the chunked path and the sample launch
  behind it returns at once for N = 0 (engine.cpp launch_sample_kernel), so
  no sample kernel reads the NaN conditioning.  The one-frame form <1, SC>
  has no such route (single_frame_chunked wants N > 0): the class is left
  off it.
* chunk_kernel's multi-frame geometries <8,8>, <16,4>, <32,2>, <20,4>, <24,4>
  on the finite class: PCM of every frame and the final state against the
  oracle, every stream's save_state against a per-frame run.
* one-frame live ticks <1,16> with 4, 2 and 1 row slices (300, 1030, 2100
  streams), deferred and eager LPC; <1,32> at 8200 streams.
* the decoder's hand-off: packets whose pitch lies below 33 and above 255
  before the decoder's clamp, through decode_frames.

A mismatch names the sequence, the frame, the field and the first indices."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cond_frames as CF
import lpcnet_amd as L
import oracle_lib as O
from test_kernel_choice import choice

pytestmark = pytest.mark.gpu

NFR, NF, FRAME = CF.NFRAMES, CF.NF, L.FRAME_SIZE
FK_WG, FK_ONE_STREAM_MAX = 4, 256      # frame_kernel<4>'s streams per workgroup; frame_kernel<1> up to this batch
LPC_CHUNK, OVERLAP_MAX = 32, 128       # frames per chunk launch; batches above this take the chunked path
PAD = L.synthetic_features(0, LPC_CHUNK)[:, :NF]  # what follows an edge sequence in a longer run


def finite_seqs(model: str) -> list:
    return [s for s in CF.MODELS[model][2] if s in CF.FINITE]


def place(n: int, B: int, wg: int) -> list:
    """n streams of a batch of B: the first, the last, both sides of the first
    boundary between workgroups of wg streams, the rest after it."""
    if B == n:
        return list(range(n))
    pos = ([0, wg - 1, wg, B - 1] + list(range(wg + 1, wg + n)))[:n]
    assert len(set(pos)) == n and max(pos) < B and (n < 4 or {0, wg - 1, wg, B - 1} <= set(pos))
    return pos


@functools.lru_cache(maxsize=None)
def synthetic(B: int, F: int) -> np.ndarray:
    """[F, B, 20] synthetic features, read-only"""
    a = np.ascontiguousarray(np.stack([L.synthetic_features(s, F)[:, :NF] for s in range(B)], 1))
    a.setflags(write=False)
    return a


def seq_features(seq: str, F: int) -> np.ndarray:
    """the 12 frames of a sequence, then PAD's"""
    return np.concatenate([CF.features_of(seq), PAD[NFR:]])[:F]


def batch_features(seqs, pos, B: int, F: int) -> np.ndarray:
    a = synthetic(B, F).copy()
    for s, p in zip(seqs, pos):
        a[:, p] = seq_features(s, F)
    return a


# -- the oracle's answers, computed once per (model, sequence) ------------------------

_oracle = {}


def oracle_runs(model: str, seqs, F: int = NFR, n: int = FRAME) -> dict:
    """{sequence: (pcm [F, n], records [F, WORDS], gru_a_state [F, 384],
    gru_b_state [F, 16])} of the live oracle; a longer run's prefix serves a
    shorter one."""
    have = [f for (m, f, k) in _oracle if m == model and k == n and f >= F]
    key = (model, min(have) if have else F, n)
    done = _oracle.setdefault(key, {})

    def one(seq):
        variant, constants, _ = CF.MODELS[model]
        o = O.Oracle(CF.model(model), variant, constants=constants)
        pcm, rec, sa, sb = [], [], [], []
        for f in seq_features(seq, key[1]):
            pcm.append(o.synthesize(f, n)[:n])
            rec.append(CF.oracle_record(o))
            a, b = o.state()
            sa.append(a)
            sb.append(b)
        return np.stack(pcm), np.stack(rec), np.stack(sa), np.stack(sb)

    todo = [s for s in seqs if s not in done]
    with ThreadPoolExecutor(8) as ex:  # ctypes calls release the GIL
        for s, r in zip(todo, ex.map(one, todo)):
            done[s] = r
    return {s: tuple(x[:F] for x in done[s]) for s in seqs}


def report(errors: list):
    assert not errors, "%d mismatches; the first: %s" % (len(errors), "\n".join(errors[:8]))


def pcm_errors(tag: str, f: int, got: np.ndarray, exp: np.ndarray) -> list:
    d = np.flatnonzero(got != exp)
    return [] if not d.size else ["%s frame %d: pcm differs from the oracle's at %d samples, first %s (got %d, expected %d)"
                                  % (tag, f, d.size, d[:6].tolist(), got[d[0]], exp[d[0]])]


def state_errors(tag: str, f, b, stream: int, exp, with_gru: bool = True) -> list:
    """get_state and save_state of a stream against the oracle's (record, gru_a_state, gru_b_state)."""
    rec, sa, sb = exp
    st = b.get_state(stream)
    got = CF.state_record(b.save_state(stream))
    err = CF.diff(tag, f, got, rec, "oracle")
    view = CF.record(st["gru_a_cond"], st["gru_b_cond"], st["lpc"], CF.field(got, "conv1_mem").view(np.float32),
                     CF.field(got, "conv2_mem").view(np.float32), st["frame_count"])
    err += CF.diff(tag, f, view, rec, "oracle (get_state)")
    if with_gru:
        for name, g, e in (("gru_a_state", st["gru_a_state"], sa), ("gru_b_state", st["gru_b_state"], sb)):
            d = np.flatnonzero(CF.bits(g) != CF.bits(e))
            if d.size:
                err.append("%s frame %s: %s differs from the oracle's at indices %s" % (tag, f, name, d[:6].tolist()))
    return err


def new_batch(model: str, B: int, chunking: bool = True):
    b = L.LPCNetBatch(B, 0, CF.model(model))
    c = CF.MODELS[model][1]
    if c is not None:
        b.set_model_constants(c[0], c[1], bool(c[2]))
    b.set_frame_chunking(chunking)
    return b


@pytest.fixture(scope="module")
def cus(require_gpu):
    """the device's CU count, as the engine reads it"""
    return choice(L, CF.model("int8"), 1, 0, 0, 0, [], [])[3]


# -- the per-frame kernel ----------------------------------------------------------------

def per_frame_batch(seqs, form: str):
    """(B, positions): fk1 = the sequences alone (one more stream if that is a
    multiple of 4), fk4 = 261 streams."""
    n = len(seqs)
    B = FK_ONE_STREAM_MAX + 5 if form == "fk4" else (n + 1 if n % FK_WG == 0 else n)
    assert B % FK_WG != 0 and (B > FK_ONE_STREAM_MAX) == (form == "fk4")
    return B, place(n, B, FK_WG) if form == "fk4" else list(range(n))


@pytest.mark.parametrize("form", ["fk1", "fk4"])
@pytest.mark.parametrize("model", list(CF.MODELS))
def test_per_frame_kernel_finite_class(require_gpu, model, form):
    """Single-frame synthesize calls: after every frame every edge stream's
    record against the fixture and the oracle, its PCM and GRU states against
    the oracle; the last frame's record is the fixture's whole record."""
    seqs = finite_seqs(model)
    B, pos = per_frame_batch(seqs, form)
    feats = batch_features(seqs, pos, B, NFR)
    exp = oracle_runs(model, seqs)
    b = new_batch(model, B, chunking=False)
    errors = []
    for f in range(NFR):
        pcm = b.synthesize(feats[f])
        for s, p in zip(seqs, pos):
            tag = "%s/%s (stream %d of %d)" % (model, s, p, B)
            e_pcm, e_rec, e_sa, e_sb = exp[s]
            errors += pcm_errors(tag, f, pcm[p], e_pcm[f])
            errors += state_errors(tag, f, b, p, (e_rec[f], e_sa[f], e_sb[f]))
            errors += CF.fixture_diff(model, s, f, CF.state_record(b.save_state(p)))
    b.close()
    report(errors)


@pytest.mark.parametrize("form", ["fk1", "fk4"])
@pytest.mark.parametrize("model", list(CF.MODELS))
def test_per_frame_kernel_frame_only_both_classes(require_gpu, model, form):
    """frame_only (N = 0) on every sequence of the model, the non-finite class
    included: NaN where the reference is NaN (the fixture pins how many),
    bit-equal elsewhere, in every frame."""
    seqs = list(CF.MODELS[model][2])
    B, pos = per_frame_batch(seqs, form)
    feats = batch_features(seqs, pos, B, NFR)
    exp = oracle_runs(model, seqs, NFR, 0)
    b = new_batch(model, B, chunking=False)
    errors = []
    for f in range(NFR):
        b.frame_only(feats[f])
        for s, p in zip(seqs, pos):
            tag = "%s/%s (stream %d of %d)" % (model, s, p, B)
            got = CF.state_record(b.save_state(p))
            errors += CF.diff(tag, f, got, exp[s][1][f], "oracle")
            errors += CF.fixture_diff(model, s, f, got)
    b.close()
    report(errors)


# -- chunk_kernel, several frames a launch ------------------------------------------------

def chunk_geometry(F: int, B: int, cus: int) -> str:
    """launch_chunk_h's rule (chunk_kernel.hip), restated"""
    cost = lambda sc, nct: ((B + sc - 1) // sc + cus - 1) // cus * nct  # noqa: E731
    if F <= 8:
        return "<8,8>"
    if F <= 16:
        return "<16,4>"
    if F <= 20 and cost(4, 5) < cost(2, 4):
        return "<20,4>"
    if F <= 24 and cost(4, 6) < cost(2, 4):
        return "<24,4>"
    return "<32,2>"


SC = {"<8,8>": 8, "<16,4>": 4, "<32,2>": 2, "<20,4>": 4, "<24,4>": 4}


def run_frames(b, feats: np.ndarray, n: int = FRAME):
    """lpcnet_batch_synthesize_frames of feats [F, B, 20]: pcm [F, B, n], (frame-kernel launches, frames they covered)"""
    F, B = feats.shape[:2]
    d_f = b.device_alloc(feats.nbytes)
    d_p = b.device_alloc(max(F * B * n * 2, 256))
    b.h2d(d_f, feats)
    b.reset_timers(2)
    b.synthesize_frames(None, d_f, d_p, F, n)
    b.sync()
    launches = (b.kernel_ms(1)[1], b.kernel_frames(1))
    b.reset_timers(0)
    pcm = np.zeros((F, B, n), np.int16)
    if n:
        b.d2h(pcm, d_p)
    b.device_free(d_f)
    b.device_free(d_p)
    return pcm, launches


def chunk_batch(geom: str, F: int, big: bool, cus: int):
    B = 2 * cus + 4 if big else OVERLAP_MAX + 5
    assert chunk_geometry(F, B, cus) == geom, (chunk_geometry(F, B, cus), geom)
    if big:  # the launch rule's own arithmetic: one round of 4-stream workgroups beats two of 2-stream ones
        cost = lambda sc, nct: ((B + sc - 1) // sc + cus - 1) // cus * nct  # noqa: E731
        assert cost(4, 5) < cost(2, 4) and cost(4, 6) < cost(2, 4)
    return B


# geometry, frames, B = 2 CUs + 4 instead of 133, model, LPCNET_NO_MULTIFRAME
CHUNKS = [
    ("<8,8>", 5, False, "int8", False),
    ("<16,4>", 12, False, "int8", False),
    ("<16,4>", 12, False, "int8", True),
    ("<16,4>", 12, False, "fp32", False),
    ("<16,4>", 12, False, "pitch_only", False),
    ("<16,4>", 12, False, "features_only", False),
    ("<16,4>", 12, False, "g092_d3", False),
    ("<16,4>", 12, False, "e2e_g09_d1", False),
    ("<32,2>", 20, False, "int8", False),
    ("<32,2>", 32, False, "int8", False),
    ("<32,2>", 32, False, "e2e_g09_d1", False),
    ("<20,4>", 20, True, "int8", False),
    ("<24,4>", 24, True, "int8", False),
    ("<24,4>", 24, True, "g092_d3", False),
]


@pytest.mark.parametrize("geom,F,big,model,no_mf", CHUNKS, ids=["%s-%d-%s%s" % (c[0], c[1], c[3], "-nomf" if c[4] else "") for c in CHUNKS])
def test_chunk_kernel_finite_class(require_gpu, monkeypatch, cus, geom, F, big, model, no_mf):
    """One lpcnet_batch_synthesize_frames call of F frames (the edge frames,
    then synthetic ones): one chunk launch covers them; PCM of every frame
    and the final state of the edge streams against the oracle, every
    stream's save_state against a per-frame run of the same batch."""
    monkeypatch.delenv("LPCNET_NO_MULTIFRAME", raising=False)
    for k in ("LPCNET_NO_CHUNK", "LPCNET_NO_OVERLAP"):
        monkeypatch.delenv(k, raising=False)
    if no_mf:
        monkeypatch.setenv("LPCNET_NO_MULTIFRAME", "1")
    B = chunk_batch(geom, F, big, cus)
    seqs = finite_seqs(model)
    pos = place(len(seqs), B, SC[geom])
    feats = batch_features(seqs, pos, B, F)
    exp = oracle_runs(model, seqs, F)
    b = new_batch(model, B)
    pcm, launches = run_frames(b, feats)
    assert launches == (1, F), launches  # one chunk launch, not F per-frame ones
    errors = []
    for s, p in zip(seqs, pos):
        tag = "%s/%s (stream %d of %d, %s)" % (model, s, p, B, geom)
        e_pcm, e_rec, e_sa, e_sb = exp[s]
        for f in range(F):
            errors += pcm_errors(tag, f, pcm[f, p], e_pcm[f])
        errors += state_errors(tag, F - 1, b, p, (e_rec[-1], e_sa[-1], e_sb[-1]))
        if F == NFR:
            errors += CF.fixture_diff(model, s, F - 1, CF.state_record(b.save_state(p)))
    snaps = [b.save_state(s) for s in range(B)]
    b.close()
    b2 = new_batch(model, B, chunking=False)
    pcm2, launches2 = run_frames(b2, feats)
    assert launches2 == (F, F), launches2
    for s in range(B):
        snap = b2.save_state(s)
        if snap != snaps[s]:
            a, c = np.frombuffer(snaps[s], CF.STATE)[0], np.frombuffer(snap, CF.STATE)[0]
            errors.append("stream %d of %d (%s): save_state differs from the per-frame run's in %s"
                          % (s, B, geom, [n for n in CF.STATE.names if a[n].tobytes() != c[n].tobytes()]))
        d = np.argwhere(pcm[:, s] != pcm2[:, s])
        if d.size:
            errors.append("stream %d of %d (%s): pcm differs from the per-frame run's first at frame %d sample %d"
                          % (s, B, geom, d[0][0], d[0][1]))
    b2.close()
    report(errors)


CHUNKS_N0 = [("<16,4>", 12, False, m) for m in CF.MODELS] + [("<8,8>", 5, False, "int8"), ("<32,2>", 32, False, "int8"),
                                                            ("<20,4>", 20, True, "int8"), ("<24,4>", 24, True, "e2e_g09_d1")]


@pytest.mark.parametrize("geom,F,big,model", CHUNKS_N0, ids=["%s-%d-%s" % (c[0], c[1], c[3]) for c in CHUNKS_N0])
def test_chunk_kernel_frame_network_only_both_classes(require_gpu, monkeypatch, cus, geom, F, big, model):
    """lpcnet_batch_synthesize_frames with N = 0 above 128 streams: the chunk
    launch runs and the sample launch behind it returns at once, so the
    non-finite class can pass through chunk_kernel.  The final record of
    every sequence against the oracle (and, after 12 frames, the fixture):
    NaN where the reference is NaN, the fixture's count of them, bit-equal
    elsewhere."""
    for k in ("LPCNET_NO_CHUNK", "LPCNET_NO_OVERLAP", "LPCNET_NO_MULTIFRAME"):
        monkeypatch.delenv(k, raising=False)
    B = chunk_batch(geom, F, big, cus)
    seqs = list(CF.MODELS[model][2])
    pos = place(len(seqs), B, SC[geom])
    feats = batch_features(seqs, pos, B, F)
    exp = oracle_runs(model, seqs, F, 0)
    b = new_batch(model, B)
    _, launches = run_frames(b, feats, 0)
    assert launches == (1, F), launches
    errors = []
    for s, p in zip(seqs, pos):
        tag = "%s/%s (stream %d of %d, %s)" % (model, s, p, B, geom)
        got = CF.state_record(b.save_state(p))
        errors += CF.diff(tag, F - 1, got, exp[s][1][-1], "oracle")
        if F == NFR:
            errors += CF.fixture_diff(model, s, F - 1, got)
    b.close()
    report(errors)


# -- one-frame live ticks -----------------------------------------------------------------

def tick_form(B: int, cus: int):
    """(streams per workgroup, row slices) of a one-frame launch: chunk_kernel.hip launch_chunk_h"""
    groups = (B + 15) // 16
    ps = 4 if 4 * groups <= cus else 2 if 2 * groups <= cus else 1
    return (16 if ps > 1 or groups <= 2 * cus else 32), ps


TICKS = [(300, "int8", False), (300, "int8", True), (1030, "int8", False), (1030, "int8", True), (2100, "int8", False),
         (2100, "int8", True), (300, "features_only", False), (1030, "pitch_only", False), (2100, "g092_d3", False),
         (300, "e2e_g09_d1", False), (300, "fp32", False), (8200, "int8", False)]


@pytest.mark.parametrize("B,model,eager", TICKS, ids=["%d-%s-%s" % (t[0], t[1], "eager" if t[2] else "deferred") for t in TICKS])
def test_live_ticks_finite_class(require_gpu, monkeypatch, cus, B, model, eager):
    """12 one-frame synthesize calls (a live server's tick) of a large batch:
    chunk_kernel<1, SC> with 4, 2 or 1 row slices, the frame's LPC deferred
    behind the sample kernel or computed first (LPCNET_LPC_EAGER=1).  PCM of
    every tick and the final state of the edge streams against the oracle."""
    for k in ("LPCNET_NO_CHUNK", "LPCNET_CK_SLICES", "LPCNET_LPC_EAGER"):
        monkeypatch.delenv(k, raising=False)
    if eager:
        monkeypatch.setenv("LPCNET_LPC_EAGER", "1")
    sc, ps = tick_form(B, cus)
    if cus == 256:
        assert (sc, ps) == {300: (16, 4), 1030: (16, 2), 2100: (16, 1), 8200: (32, 1)}[B]
    seqs = finite_seqs(model)
    pos = place(len(seqs), B, sc)
    feats = batch_features(seqs, pos, B, NFR)
    exp = oracle_runs(model, seqs)
    b = new_batch(model, B)
    errors = []
    for f in range(NFR):
        pcm = b.synthesize(feats[f])
        for s, p in zip(seqs, pos):
            errors += pcm_errors("%s/%s (stream %d of %d, <1,%d> x %d slices)" % (model, s, p, B, sc, ps), f, pcm[p], exp[s][0][f])
    for s, p in zip(seqs, pos):
        tag = "%s/%s (stream %d of %d, <1,%d> x %d slices)" % (model, s, p, B, sc, ps)
        e_pcm, e_rec, e_sa, e_sb = exp[s]
        errors += state_errors(tag, NFR - 1, b, p, (e_rec[-1], e_sa[-1], e_sb[-1]))
        errors += CF.fixture_diff(model, s, NFR - 1, CF.state_record(b.save_state(p)))
    b.close()
    report(errors)


# -- the decoder's hand-off -----------------------------------------------------------------

def packet(c0_id, main_pitch, modulation, corr_id, vq_end, vq_mid, interp_id) -> bytes:
    """decode_packet's fields (lpcnet_dec.c:81-93), MSB first"""
    v = 0
    for val, n in ((c0_id, 7), (main_pitch, 6), (modulation, 3), (corr_id, 2), (vq_end[0], 10), (vq_end[1], 10),
                   (vq_end[2], 10), (vq_mid, 13), (interp_id, 3)):
        assert 0 <= val < (1 << n)
        v = (v << n) | int(val)
    return v.to_bytes(8, "big")


@pytest.mark.parametrize("B", [96, 133])
def test_decoder_hands_over_clamped_pitch(require_gpu, B):
    """Packets with main_pitch 0 and 63 and modulation 0 (unvoiced) and 7: the
    pitch lies below 33 and above 255 before the decoder's clamp, so
    features[18] arrives at both of its extremes and the frame network reads
    embedding rows 33 and 255.  decode_frames (96 streams: overlapped
    per-frame path, 133: chunked) against the oracle's decoder."""
    blob = L.synthetic_model(1, L.VARIANT_INT8, codebooks=True)
    P = 3
    rng = np.random.RandomState(CF.SEED + B)
    pk = np.zeros((P, B, 8), np.uint8)
    for p in range(P):
        for s in range(B):
            mp, mod = [(0, 0), (63, 7), (0, 7), (63, 0)][(s + p) % 4]
            pk[p, s] = np.frombuffer(packet(rng.randint(128), mp, mod, rng.randint(4), rng.randint(1024, size=3),
                                            rng.randint(8192), rng.randint(8)), np.uint8)
    check = sorted({0, 1, 2, 3, 4, B // 2, B - 1})
    want, rows = {}, set()
    for s in check:
        o = O.Oracle(blob, 0)
        for p in range(P):
            rows |= {CF.pitch_ref(x) for x in o.decode_packet(bytes(pk[p, s]))[:, 18]}
        o = O.Oracle(blob, 0)
        want[s] = np.stack([o.decode(bytes(pk[p, s])) for p in range(P)]).reshape(4 * P, FRAME)
    assert {33, 255} <= rows, rows
    b = L.LPCNetBatch(B, 0, blob)
    d_pk = b.device_alloc(pk.nbytes)
    d_pcm = b.device_alloc(4 * P * B * FRAME * 2)
    b.h2d(d_pk, pk)
    b.decode_frames(d_pk, d_pcm, P)
    b.sync()
    pcm = np.zeros((4 * P, B, FRAME), np.int16)
    b.d2h(pcm, d_pcm)
    b.device_free(d_pk)
    b.device_free(d_pcm)
    b.close()
    errors = []
    for s in check:
        for f in range(4 * P):
            errors += pcm_errors("decoder stream %d of %d" % (s, B), f, pcm[f, s], want[s][f])
    report(errors)
