"""What the step layer queues, call by call: per call its sample-kernel and
frame-kernel launch counts and frames (lpcnet_batch_kernel_ms / _kernel_frames,
regions 0 and 1, timers at 2) and the CRC of its PCM, as JSON, for comparing
two builds:

    python tools/launch_counts.py out.json
"""
import json
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lpcnet_amd as L

out = {}


def counts(b):
    b.sync()
    return [b.kernel_ms(0)[1], b.kernel_ms(1)[1], b.kernel_frames(0), b.kernel_frames(1)]


def feats(B, F):
    return np.ascontiguousarray(np.stack([L.synthetic_features(s % 7, F)[:, :20] for s in range(B)], axis=1), np.float32)


blob = L.synthetic_model(1, L.VARIANT_INT8, codebooks=True)
for B in (4, 129, 1024):
    f = feats(B, 3)
    b = L.LPCNetBatch(B, 0, blob)
    for name, call in (("synthesize", lambda: b.synthesize(f[0])), ("synthesize2", lambda: b.synthesize(f[1])),
                       ("run_frame_network", lambda: b.run_frame_network(f[2], True)),
                       ("synthesize_tail", lambda: b.synthesize_tail_impl(np.zeros((B, 80), np.int16))),
                       ("decode", lambda: b.decode((np.arange(B * 8).reshape(B, 8) * 7 % 251).astype(np.uint8)))):
        b.reset_timers(2)
        r = call()
        c = counts(b)
        out[f"{name} B={B}"] = c + [zlib.crc32(np.ascontiguousarray(r).tobytes()) if r is not None else None]
    b.close()
for B, chunk in ((4, True), (4, False), (129, True), (129, False)):
    F = 40
    f = feats(B, F)
    b = L.LPCNetBatch(B, 0, blob)
    b.set_frame_chunking(chunk)
    d_f, d_p = b.device_alloc(f.nbytes), b.device_alloc(F * B * 160 * 2)
    b.h2d(d_f, f)
    b.reset_timers(2)
    b.synthesize_frames(None, d_f, d_p, F, 160)
    c = counts(b)
    pcm = np.zeros((F, B, 160), np.int16)
    b.d2h(pcm, d_p)
    out[f"synthesize_frames40 B={B} chunking={int(chunk)}"] = c + [zlib.crc32(pcm.tobytes())]
    b.close()
for k, v in out.items():
    print(k, v)
json.dump(out, open(sys.argv[1], "w"), indent=1)
