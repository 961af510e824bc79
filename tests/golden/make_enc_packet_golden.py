#!/usr/bin/env python3
"""Generates tests/golden/enc_packets.npz (run where oracle/_ref is built).

The 23 int16 edge-case signals of tests/feat_signals.py plus one all-zero
stream, 24 frames = 6 packets each, through tests/enc_packet_ref.py (the
reference's own compiled freq.c / pitch.c composed with the restated glue,
process_superframe and quantisers of lpcnet_enc.c), with the ceps codebooks of
synthetic_model(1, VARIANT_INT8, codebooks=True):

  names          [24]
  pcm            [24, 24, 160] int16
  cb1 cb2 cb3 cbd  the codebooks, flat float32
  packets        [24, 6, 8] uint8     lpcnet_encode
  qfeat          [24, 6, 4, 36]       st->features after each lpcnet_encode
  nearest1       [24, 6]              the first stage's nearest entry (coverage:
                                      the m-best search matters where it is not
                                      the packet's vq_end0)
  unpacked       [24, 6, 2] int32     corr_id and modulation as the encoder found
                                      them: the packet keeps corr_id & 3 and,
                                      unvoiced, no modulation
  state_enc      [24, n] uint8        EncPacketRef.state_bytes() after packet 5
  ufeat          [24, 6, 4, 36]       lpcnet_compute_features, a state of its own
  state_feat     [24, n] uint8
  tie_packets    [24, 6, 8]           lpcnet_encode with tie_codebooks(): every
                                      distance has an equal partner
  mix_single     [24, 3, 4, 36]       one state driven alternately: four
  mix_packets    [24, 3, 8]           single-frame extractions (packets 0, 2, 4's
  mix_qfeat      [24, 3, 4, 36]       PCM), then lpcnet_encode (packets 1, 3, 5's)
  mix_state      [24, n] uint8

Usage: python3 tests/golden/make_enc_packet_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import enc_packet_ref as P  # noqa: E402
import feat_signals as FS  # noqa: E402
import lpcnet_amd as L  # noqa: E402

NAMES = FS.INT16 + ["zero"]


def arrays() -> dict:
    pcm = np.concatenate([FS.make_all()[0], np.zeros((1, FS.NFRAMES, FS.FRAME), np.int16)])
    cb = P.blob_codebooks(L.synthetic_model(1, L.VARIANT_INT8, codebooks=True))
    tcb = P.tie_codebooks(cb)
    out = {k: [] for k in ("packets", "qfeat", "nearest1", "unpacked", "state_enc", "ufeat", "state_feat", "tie_packets", "mix_single",
                           "mix_packets", "mix_qfeat", "mix_state")}
    for sig in pcm:
        p640 = sig.reshape(P.NPACKETS, 640)
        r = P.EncPacketRef(cb)
        pk, qf, n1, up = [], [], [], []
        for x in p640:
            b, f = r.encode(x)
            pk.append(np.frombuffer(b, np.uint8))
            qf.append(f)
            n1.append(r.info["nearest1"])
            up.append([r.info["corr_id"], r.info["modulation"]])
        out["packets"].append(np.stack(pk))
        out["qfeat"].append(np.stack(qf))
        out["nearest1"].append(np.array(n1, np.int32))
        out["unpacked"].append(np.array(up, np.int32))
        out["state_enc"].append(np.frombuffer(r.state_bytes(), np.uint8))
        r = P.EncPacketRef()
        out["ufeat"].append(np.stack([r.compute_features4(x) for x in p640]))
        out["state_feat"].append(np.frombuffer(r.state_bytes(), np.uint8))
        r = P.EncPacketRef(tcb)
        out["tie_packets"].append(np.stack([np.frombuffer(r.encode(x)[0], np.uint8) for x in p640]))
        r = P.EncPacketRef(cb)
        ms, mp, mq = [], [], []
        for k in range(0, P.NPACKETS, 2):
            ms.append(np.stack([r.frame(fr) for fr in p640[k].reshape(4, 160)]))
            b, f = r.encode(p640[k + 1])
            mp.append(np.frombuffer(b, np.uint8))
            mq.append(f)
        out["mix_single"].append(np.stack(ms))
        out["mix_packets"].append(np.stack(mp))
        out["mix_qfeat"].append(np.stack(mq))
        out["mix_state"].append(np.frombuffer(r.state_bytes(), np.uint8))
    a = {k: np.stack(v) for k, v in out.items()}
    a.update(names=np.array(NAMES), pcm=pcm, cb1=cb["ceps_codebook1"], cb2=cb["ceps_codebook2"], cb3=cb["ceps_codebook3"],
             cbd=cb["ceps_codebook_diff4"])
    return a


def main():
    assert P.E.have_ref(), "oracle/_ref/libref_kernels.so missing: run `make -C oracle` with the reference tree present"
    a = arrays()
    assert np.isfinite(a["ufeat"]).all() and np.isfinite(a["qfeat"]).all()
    np.savez_compressed(P.GOLDEN, **a)
    print("wrote %s: %d signals, %d bytes" % (P.GOLDEN, len(NAMES), os.path.getsize(P.GOLDEN)))
    f = np.array([[list(P.unpack(p).values()) for p in s] for s in a["packets"]])
    print("  voiced", sorted(set((f[..., 2] != 0).ravel().tolist())), "vq_mid sign", sorted(set((f[..., 7] >= 4096).ravel().tolist())),
          "class", sorted(set((f[..., 7] & 3).ravel().tolist())), "interp", sorted(set(f[..., 8].ravel().tolist())),
          "mbest matters in", int((f[..., 4] != a["nearest1"]).sum()), "zero main_pitch", f[-1, :, 1].tolist())


if __name__ == "__main__":
    main()
