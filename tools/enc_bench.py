#!/usr/bin/env python3
"""Side measurement: the 1.6 kb/s encoder's kernel time per packet, split into
its four analysis launches and enc_kernel.hip, beside four single-frame
extractor calls at the same batch ("1.6 kb/s encoder").

    python tools/enc_bench.py [--batches 1024,8192,32768] [--out FILE]

Per batch: tools/feat_bench.py's extractor measurement (a batch without a
model, 100 ms preheat, 50 timed single-frame calls, which = 3), then on a
batch with the synthetic model's codebooks a 100 ms preheat with the encoder
itself and 24 timed packets on device-resident PCM (lpcnet_batch_kernel_ms
which = 4 and 5), every stream active, feat_bench's signals (four frames of
voiced, noisy and silent streams).  One JSON line per batch, with the packet's
kernel time against the 40 ms it covers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import feat_bench  # noqa: E402
import lpcnet_amd as L  # noqa: E402

PACKETS = 24


def measure(blob: bytes, B: int, preheat_ms: float) -> dict:
    pcm = feat_bench.signals(B)  # [4, B, 160]: one packet
    b = L.LPCNetBatch(B, 0, blob)
    d_pcm = b.device_alloc(pcm.nbytes)
    d_pk = b.device_alloc(B * 8)
    d_feat = b.device_alloc(4 * B * L.NB_FEATURES * 4)
    b.h2d(d_pcm, pcm)
    t_end = time.perf_counter() + preheat_ms * 1e-3
    while time.perf_counter() < t_end:
        b.encode_device(d_pcm, d_pk, d_feat, L.NB_FEATURES, None, 1)
        b.sync()
    b.reset_timers(1)
    t0 = time.perf_counter()
    for _ in range(PACKETS):
        b.encode_device(d_pcm, d_pk, d_feat, L.NB_FEATURES, None, 1)
    b.sync()
    wall = (time.perf_counter() - t0) / PACKETS
    ms, n = b.kernel_ms(4)
    ms_enc, n_enc = b.kernel_ms(5)
    assert n == 5 * PACKETS and n_enc == PACKETS and b.kernel_frames(4) == 4 * PACKETS
    pk = np.zeros((B, 8), np.uint8)
    b.d2h(pk, d_pk)
    for d in (d_pcm, d_pk, d_feat):
        b.device_free(d)
    b.close()
    return {"encoder_kernel_ms_per_packet": round(ms / PACKETS, 5),
            "analysis_ms_per_packet": round((ms - ms_enc) / PACKETS, 5),
            "enc_kernel_ms_per_packet": round(ms_enc / PACKETS, 5),
            "encoder_wall_ms_per_packet": round(wall * 1e3, 5),
            "distinct_packets": int(len({bytes(p) for p in pk}))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,8192,32768")
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("enc_bench: no HIP device visible")
    blob = L.synthetic_model(1, L.VARIANT_INT8, codebooks=True)
    lines = []
    for B in [int(v) for v in a.batches.split(",")]:
        r = {"streams": B}
        x = feat_bench.measure(B, a.preheat_ms)
        r["four_extractor_calls_ms"] = round(4 * x["extractor_kernel_ms_per_call"], 5)
        r.update(measure(blob, B, a.preheat_ms))
        r["packet_ms"] = 40.0
        r["real_time_margin"] = round(40.0 / r["encoder_kernel_ms_per_packet"], 2)
        if os.environ.get("LPCNET_LIB_VARIANT"):
            r["lib_variant"] = os.environ["LPCNET_LIB_VARIANT"]
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
