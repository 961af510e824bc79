#!/usr/bin/env python3
"""Writes tests/golden/burg_cepstrum.npz: burg_cepstral_analysis of the 29
edge-case signals of tests/feat_signals.py (their PCM stays in
enc_features_edge.npz) and of four sine signals (tests/burg_ref.py SINES,
PCM stored here), 24 frames each, from the reference's own compiled freq.c /
burg.c (oracle/_ref/libref_kernels.so, built by oracle/Makefile).

    python tests/golden/make_burg_golden.py

Per signal: ceps [24, 36]; per half-frame the 16 coefficients and the
residual energy of silk_burg_analysis called directly on its burg_in, and
stop_order: the order at which the recursion hit the gain clamp (the clamp
zeroes every later coefficient), 16 if it never did, 0 if A is all zero.
Data only; TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import burg_ref as R  # noqa: E402
import feat_signals as FS  # noqa: E402


def main():
    if not R.have_ref():
        sys.exit("make_burg_golden: oracle/_ref/libref_kernels.so is not built (make -C oracle)")
    sines = np.stack([R.make_sine(n) for n in R.SINES]).reshape(len(R.SINES), FS.NFRAMES, FS.FRAME)
    S = len(R.NAMES)
    ceps = np.zeros((S, FS.NFRAMES, 36), np.float32)
    A = np.zeros((S, FS.NFRAMES, 2, 16), np.float32)
    nrg = np.zeros((S, FS.NFRAMES, 2), np.float32)
    stop = np.zeros((S, FS.NFRAMES, 2), np.int32)
    for s, name in enumerate(R.NAMES):
        pcm = sines[list(R.SINES).index(name)] if name in R.SINES else FS.pcm_of(name)
        for f in range(FS.NFRAMES):
            ceps[s, f], A[s, f], nrg[s, f], stop[s, f] = R.ref_frame(pcm[f])
        print("%-12s stop orders %s" % (name, dict(zip(*np.unique(stop[s], return_counts=True)))))
    assert np.isfinite(ceps).all() and np.isfinite(A).all() and np.isfinite(nrg).all()
    np.savez_compressed(R.GOLDEN, names=np.array(R.NAMES), pcm_sine=sines, ceps=ceps, A=A, nrg=nrg, stop_order=stop)
    print("wrote %s (%d bytes)" % (R.GOLDEN, os.path.getsize(R.GOLDEN)))


if __name__ == "__main__":
    main()
