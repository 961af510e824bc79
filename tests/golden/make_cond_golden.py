#!/usr/bin/env python3
"""Generates tests/golden/cond_edge.npz: the edge-case feature frames of
tests/cond_frames.py through the CPU oracle's frame network
(Oracle.synthesize(f, 0), then the frame's outputs and conv memories), for
every (model, sequence) of cond_frames.RUNS.

Per run and frame: the SHA-256 of the canonical record, gru_b_cond, lpc and
the number of NaN values; per run the whole record of the last frame.  Where
oracle/_ref is built the oracle runs on the reference's own compiled kernels
and the port kernels are checked against them; the file is the same either
way (tests/test_cond_frames_ref.py).  The archive is written with fixed
member timestamps, so a re-run reproduces it byte for byte.

Usage: python3 tests/golden/make_cond_golden.py [output.npz]
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cond_frames as CF  # noqa: E402
import oracle_lib as O  # noqa: E402


def run(model_name: str, feats: np.ndarray, kernels=None, avx2_build: bool = False) -> np.ndarray:
    """records [NFRAMES, WORDS] of one sequence on one model"""
    variant, constants, _ = CF.MODELS[model_name]
    o = O.Oracle(CF.model(model_name), variant, kernels, constants, avx2_build=avx2_build)
    out = []
    for f in feats:
        o.synthesize(f, 0)
        out.append(CF.oracle_record(o))
    return np.stack(out)


def lpc_finite(feats: np.ndarray) -> bool:
    k = O.kernel_table(O.ref_kernels() if O.have_ref() else O.port_kernels())
    out = np.zeros(16, np.float32)
    for f in feats:
        c = np.ascontiguousarray(f, np.float32)
        k.lpc_from_cepstrum(out.ctypes.data, c.ctypes.data)
        if not np.isfinite(out).all():
            return False
    return True


def arrays() -> dict:
    """What cond_edge.npz holds (tests/cond_frames.py: fixture())."""
    feats = np.stack([CF.make(n, lpc_finite) for n in CF.NAMES])
    models = list(CF.MODELS)
    runs, recs = [], []
    for m, s in CF.RUNS:
        r = run(m, feats[CF.NAMES.index(s)], O.ref_kernels())
        if O.have_ref():
            assert np.array_equal(r, run(m, feats[CF.NAMES.index(s)])), ("port kernels differ from the reference's", m, s)
        runs.append((models.index(m), CF.NAMES.index(s)))
        recs.append(r)
    recs = np.stack(recs)  # [R, 12, WORDS]
    digests = np.array([[np.frombuffer(CF.digest(f), np.uint8) for f in r] for r in recs])
    nans = np.array([[CF.nan_count(f) for f in r] for r in recs], np.int16)
    finite = np.isfinite(recs[:, :, :CF.WORDS - 1].view(np.float32)).all(-1)
    return dict(names=np.array(CF.NAMES), features=feats, models=np.array(models), runs=np.array(runs, np.int16),
                digests=digests, gru_b_cond=np.ascontiguousarray(CF.field(recs, "gru_b_cond")),
                lpc=np.ascontiguousarray(CF.field(recs, "lpc")), nan_count=nans, finite=finite, last=np.ascontiguousarray(recs[:, -1]))


def save(path: str, a: dict) -> None:
    """np.savez_compressed with fixed member timestamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(a):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else CF.GOLDEN
    a = arrays()
    fin = [r for r, (m, s) in enumerate(CF.RUNS) if s in CF.FINITE]
    for r in fin:
        assert a["finite"][r].all(), "%s/%s is not finite in frames %s" % (CF.RUNS[r] + (np.flatnonzero(~a["finite"][r]).tolist(),))
    sep = CF.form_separation(a["features"][CF.NAMES.index("pitch_forms"), :, 18])
    for form, vals in sep.items():
        inside = [v for v in vals if CF.DECODER_RANGE[0] <= v <= CF.DECODER_RANGE[1]]
        assert len(vals) >= 2 and inside, "pitch form %s is not separated" % form
        print("  %-10s separated at f18 = %s" % (form, ", ".join("%.9g" % v for v in vals)))
    save(path, a)
    print("wrote %s: %d sequences, %d runs, %d bytes (%s the reference's kernels)"
          % (path, len(CF.NAMES), len(CF.RUNS), os.path.getsize(path), "on" if O.have_ref() else "without"))


if __name__ == "__main__":
    main()
