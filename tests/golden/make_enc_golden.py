#!/usr/bin/env python3
"""Generates tests/golden/enc_features.npz and
tests/golden/enc_features_edge.npz (run where oracle/_ref is built).

Five int16 signals x 12 frames and the [12][36] features of each, computed by
tests/enc_ref.py: the reference's own compiled freq.c / pitch.c
(oracle/_ref/libref_kernels.so) composed with the restated glue of
lpcnet_enc.c's single-frame path.

  pulse80    a resonated pulse train of period 80 plus low noise
  pulse57    the same at period 57
  silence    all zero (every Viterbi maximum tied: strict > decides)
  noise      uniform noise in [-3000, 3000]
  square100  a full-scale (+-32767) square wave of period 100

enc_features_edge.npz: the 23 int16 and 4 float32 edge-case signals of
tests/feat_signals.py x 24 frames, with the features of every frame, the
SHA-256 of EncRef.state_bytes() after every frame and the state after the
last one.

Usage: python3 tests/golden/make_enc_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import enc_ref as E  # noqa: E402
import feat_signals as FS  # noqa: E402

NFRAMES = 12
N = NFRAMES * E.FRAME_SIZE


def pulse_train(period: int, rng) -> np.ndarray:
    """Pulses of 6000 every `period` samples through the two-pole resonator
    y[n] = x[n] + 1.2 y[n-1] - 0.72 y[n-2], plus uniform noise in [-20, 20]."""
    x = np.zeros(N)
    x[::period] = 6000.0
    y = np.zeros(N)
    for n in range(N):
        y[n] = x[n] + (1.2 * y[n - 1] if n >= 1 else 0.0) - (0.72 * y[n - 2] if n >= 2 else 0.0)
    y += rng.integers(-20, 21, N)
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


def signals() -> np.ndarray:
    rng = np.random.default_rng(20261019)
    sq = np.where((np.arange(N) % 100) < 50, 32767, -32767).astype(np.int16)
    s = [pulse_train(80, rng), pulse_train(57, rng), np.zeros(N, np.int16),
         rng.integers(-3000, 3001, N).astype(np.int16), sq]
    return np.stack(s).reshape(len(s), NFRAMES, E.FRAME_SIZE)


def main():
    assert E.have_ref(), "oracle/_ref/libref_kernels.so missing: run `make -C oracle` with the reference tree present"
    pcm = signals()
    feats = np.stack([E.run(p) for p in pcm])
    assert np.isfinite(feats).all()
    np.savez_compressed(E.GOLDEN, pcm=pcm, features=feats, names=np.array(E.SIGNALS))
    print("wrote %s: pcm %s, features %s, %d bytes" % (E.GOLDEN, pcm.shape, feats.shape, os.path.getsize(E.GOLDEN)))
    for n, f in zip(E.SIGNALS, feats):
        print("  %-10s pitch %s corr %s" % (n, np.round(f[-3:, 18], 2), np.round(f[-3:, 19], 3)))


def edge_arrays() -> dict:
    """What enc_features_edge.npz holds (tests/feat_signals.py: fixture())."""
    pcm_i16, pcm_f32 = FS.make_all()
    feats, digests, states = [], [], []
    for pcm in list(pcm_i16) + list(pcm_f32):
        r = E.EncRef()
        f, d = [], []
        for frame in pcm:
            f.append(r.frame(frame))
            d.append(np.frombuffer(FS.digest(r.state_bytes()), np.uint8))
        feats.append(np.stack(f))
        digests.append(np.stack(d))
        states.append(np.frombuffer(r.state_bytes(), np.uint8))
    return dict(pcm_i16=pcm_i16, pcm_f32=pcm_f32, features=np.stack(feats), digests=np.stack(digests),
                state=np.stack(states), names=np.array(FS.NAMES))


def main_edge():
    a = edge_arrays()
    assert np.isfinite(a["features"]).all()
    np.savez_compressed(FS.GOLDEN, **a)
    print("wrote %s: %d signals, %d bytes" % (FS.GOLDEN, len(FS.NAMES), os.path.getsize(FS.GOLDEN)))


if __name__ == "__main__":
    main()
    main_edge()
