#!/usr/bin/env python3
"""Side measurement: the DRED RDO-VAE's kernel time per encoder call and per
decode_all of 1, 10 and 50 latents ("rdovae_kernel").

    python tools/rdovae_bench.py [--batches 1024,8192] [--latents 1,10,50] [--out FILE]

Per batch, on the synthetic model's RDO-VAE records in dump_rdovae.py's default
shape and on device-resident buffers, every stream active: a 100 ms preheat
with the call itself, then CALLS timed calls (lpcnet_batch_kernel_ms which = 8
for the encoder, 9 for the decoder).  An encoder call covers two frames, 20 ms
of speech per stream; a decode_all of n latents produces 4 n frames, 40 n ms.
The encoder and a one-latent decode_all run the same eight-layer stack; they
differ in their heads (the conv's 4 T columns and gdense1's T against
dec_final's T), so their difference bounds the conv's share.  One JSON line
per batch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lpcnet_amd as L  # noqa: E402

CALLS = 20
NF = L.NB_FEATURES


def timed(b, which: int, call, preheat_ms: float, calls: int = CALLS) -> float:
    """Kernel ms per call of ``call`` after the preheat."""
    t_end = time.perf_counter() + preheat_ms * 1e-3
    while time.perf_counter() < t_end:
        call()
        b.sync()
    b.reset_timers(1)
    for _ in range(calls):
        call()
    b.sync()
    ms, n = b.kernel_ms(which)
    assert n == calls, (n, calls)
    b.reset_timers(0)
    return ms / calls


def measure(blob: bytes, B: int, latents, preheat_ms: float) -> dict:
    d = L.rdovae_dims(blob)
    Ld, S = d["dec"]["L"], d["dec"]["S"]
    nmax = max(latents)
    b = L.LPCNetBatch(B, 0, blob)
    base = np.stack([L.synthetic_features(s, 2)[:, :NF] for s in range(64)], 1)  # [2, 64, 20]
    feats = np.ascontiguousarray(base[:, np.arange(B) % 64])  # [2, B, 20]
    rng = np.random.RandomState(5)
    d_feat = b.device_alloc(feats.nbytes)
    d_lat = b.device_alloc(B * nmax * Ld * 4)
    d_st = b.device_alloc(B * S * 4)
    d_z = b.device_alloc(B * d["enc"]["L"] * 4)
    d_s = b.device_alloc(B * d["enc"]["S"] * 4)
    d_out = b.device_alloc(B * nmax * 4 * NF * 4)
    b.h2d(d_feat, np.ascontiguousarray(feats, np.float32))
    b.h2d(d_st, rng.uniform(-0.9, 0.9, (B, S)).astype(np.float32))
    r = {}
    enc = timed(b, 8, lambda: b.rdovae_encode_device(d_feat, d_z, d_s, NF), preheat_ms)
    r["encoder_kernel_ms_per_call"] = round(enc, 5)
    r["encoder_real_time_margin"] = round(20.0 / enc, 2)
    for n in latents:
        b.h2d(d_lat, (0.75 * rng.randn(B, n, Ld)).astype(np.float32))
        ms = timed(b, 9, lambda: b.rdovae_decode_all_device(d_st, d_lat, d_out, n), preheat_ms, CALLS if n < 50 else 5)
        r["decode_all_%d_kernel_ms" % n] = round(ms, 5)
        r["decode_all_%d_ms_per_latent" % n] = round(ms / n, 5)
        r["decode_all_%d_real_time_margin" % n] = round(40.0 * n / ms, 2)
    r["encoder_minus_one_latent_ms"] = round(enc - r["decode_all_%d_kernel_ms" % min(latents)] / min(latents), 5)
    out = np.zeros((B, 4 * latents[-1], NF), np.float32)
    b.d2h(out, d_out)  # the last decode_all's frames
    for p in (d_feat, d_lat, d_st, d_z, d_s, d_out):
        b.device_free(p)
    b.close()
    assert np.isfinite(out).all() and np.abs(out).max() > 1e-3
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--latents", default="1,10,50")
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("rdovae_bench: no HIP device visible")
    blob = L.synthetic_model(1, L.VARIANT_INT8, rdovae=True)
    latents = [int(v) for v in a.latents.split(",")]
    lines = []
    for B in [int(v) for v in a.batches.split(",")]:
        r = {"streams": B}
        r.update(measure(blob, B, latents, a.preheat_ms))
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
