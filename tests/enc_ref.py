"""CPU reference of the single-frame feature extractor
(lpcnet_compute_single_frame_features: preemphasis, compute_frame_features,
process_single_frame; lpcnet_enc.c:872-880, 488-577, 814-870 with pcount = 0):
one stream's LPCNetEncState, composed in float32 numpy around the reference's
own compiled freq.c / pitch.c (oracle/_ref/libref_kernels.so: apply_window,
forward_transform, lpcn_compute_band_energy, dct, lpc_from_cepstrum,
celt_pitch_xcorr).  The glue between those calls is restated here line by
line (lpcnet_enc.c itself needs the generated nnet_data.h).  Shared by
tests/test_features_ref.py, tests/test_gpu_features.py and
tests/golden/make_enc_golden.py.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

import oracle_lib as O

F = np.float32
FRAME_SIZE = 160          # freq.h:42
OVERLAP_SIZE = 160        # freq.h:43
TRAINING_OFFSET = 80      # freq.h:44
WINDOW_SIZE = 320         # freq.h:45
FREQ_SIZE = 161           # freq.h:46
NB_BANDS = 18             # freq.h:48
LPC_ORDER = 16            # freq.h:32
PREEMPHASIS = F(0.85)     # freq.h:34
PITCH_MIN_PERIOD = 32     # lpcnet_private.h:14
PITCH_MAX_PERIOD = 256    # lpcnet_private.h:15
NB_TOTAL_FEATURES = 36
NSTATES = PITCH_MAX_PERIOD - PITCH_MIN_PERIOD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enc_features.npz")
SIGNALS = ["pulse80", "pulse57", "silence", "noise", "square100"]

_lib = None


def have_ref() -> bool:
    return O.have_ref()


def lib():
    """The reference's compiled kernels (freq.c, pitch.c) with argument types."""
    global _lib
    if _lib is None:
        l = C.CDLL(O.REF_SO)
        vp, i = C.c_void_p, C.c_int
        l.apply_window.argtypes = [vp]
        l.forward_transform.argtypes = [vp, vp]
        l.lpcn_compute_band_energy.argtypes = [vp, vp]
        l.dct.argtypes = [vp, vp]
        l.lpc_from_cepstrum.argtypes = [vp, vp]
        l.lpc_from_cepstrum.restype = C.c_float
        l.celt_pitch_xcorr.argtypes = [vp, vp, vp, i, i]
        for f in (l.apply_window, l.forward_transform, l.lpcn_compute_band_energy, l.dct, l.celt_pitch_xcorr):
            f.restype = None
        _lib = l
    return _lib


def half_window() -> np.ndarray:
    """The reference's half_window table (lpcnet_tables.c:207)."""
    return np.ctypeslib.as_array((C.c_float * OVERLAP_SIZE).in_dll(lib(), "half_window")).copy()


def _max16(a, b):
    return a if a > b else b  # arch.h:73


def _inner_prod(x: np.ndarray, y: np.ndarray) -> np.float32:
    """celt_inner_prod (pitch.h:109-117): xy = xy + x[i]*y[i] in float, in order."""
    xy = F(0)
    for p in (x * y):  # float32 products
        xy = F(xy + p)
    return xy


class EncRef:
    """The fields of LPCNetEncState (lpcnet_private.h) the single-frame path uses."""

    def __init__(self):
        self.l = lib()
        self.reset()

    def reset(self):
        """lpcnet_encoder_init (lpcnet_enc.c:471-475): memset 0."""
        self.analysis_mem = np.zeros(OVERLAP_SIZE, F)
        self.mem_preemph = F(0)
        self.pitch_mem = np.zeros(LPC_ORDER, F)
        self.pitch_filt = F(0)
        self.exc_buf = np.zeros(PITCH_MAX_PERIOD + FRAME_SIZE, F)  # the part of PITCH_BUF_SIZE this path touches
        self.xc = np.zeros((2, PITCH_MAX_PERIOD), F)  # rows 2, 3 (pcount = 0)
        self.frame_weight = np.zeros(2, F)            # entries 2, 3
        self.pitch_max_path = np.zeros((2, PITCH_MAX_PERIOD), F)
        self.pitch_max_path_all = F(0)
        self.best_i = 0
        self.lpc = np.zeros(LPC_ORDER, F)
        self.features = np.zeros(NB_TOTAL_FEATURES, F)

    def state_bytes(self) -> bytes:
        """What crosses frames, in the layout of the engine's per-stream
        snapshot (lpcnet_batch_features_save_state)."""
        return (self.analysis_mem.tobytes() + self.exc_buf[FRAME_SIZE:].tobytes() + self.pitch_max_path[0].tobytes()
                + self.pitch_mem.tobytes() + np.array([self.mem_preemph, self.pitch_filt, self.pitch_max_path_all], F).tobytes()
                + np.array([self.best_i], np.int32).tobytes())

    # -- lpcnet_enc.c:872-880 ------------------------------------------------
    def preemphasis(self, x: np.ndarray) -> np.ndarray:
        """y[i] = x[i] + mem; mem = -coef*x[i]: only mem crosses the frame."""
        mem = np.concatenate([[self.mem_preemph], (-PREEMPHASIS) * x[:-1]]).astype(F)
        self.mem_preemph = F((-PREEMPHASIS) * x[-1])
        return (x + mem).astype(F)

    # -- lpcnet_enc.c:488-496 ------------------------------------------------
    def frame_analysis(self, inp: np.ndarray):
        x = np.concatenate([self.analysis_mem, inp]).astype(F)  # :490-491
        self.analysis_mem = inp[FRAME_SIZE - OVERLAP_SIZE:].copy()  # :492
        self.l.apply_window(x.ctypes.data)
        X = np.zeros(2 * FREQ_SIZE, F)
        self.l.forward_transform(X.ctypes.data, x.ctypes.data)
        Ex = np.zeros(NB_BANDS, F)
        self.l.lpcn_compute_band_energy(Ex.ctypes.data, X.ctypes.data)
        return Ex

    # -- lpcnet_enc.c:498-577 ------------------------------------------------
    def compute_frame_features(self, inp: np.ndarray):
        aligned_in = np.zeros(FRAME_SIZE, F)
        aligned_in[:TRAINING_OFFSET] = self.analysis_mem[OVERLAP_SIZE - TRAINING_OFFSET:]  # :510, before :492 replaces it
        Ex = self.frame_analysis(inp)
        logMax, follow = F(-2), F(-2)
        Ly = np.zeros(NB_BANDS, F)
        for i in range(NB_BANDS):  # :514-520
            ly = F(math.log10(1e-2 + float(Ex[i])))  # double add, double log10, rounded to float
            ly = _max16(F(logMax - F(8)), _max16(F(follow - F(2.5)), ly))
            logMax = _max16(logMax, ly)
            follow = _max16(F(follow - F(2.5)), ly)
            Ly[i] = ly
        ceps = np.zeros(NB_BANDS, F)
        self.l.dct(ceps.ctypes.data, Ly.ctypes.data)  # :521
        ceps[0] = F(ceps[0] - F(4))  # :522
        self.features[:NB_BANDS] = ceps
        lpc = np.zeros(LPC_ORDER, F)
        self.l.lpc_from_cepstrum(lpc.ctypes.data, ceps.ctypes.data)  # :523
        self.lpc = lpc
        self.features[NB_BANDS + 2:] = lpc  # :524
        self.exc_buf[:PITCH_MAX_PERIOD] = self.exc_buf[FRAME_SIZE:FRAME_SIZE + PITCH_MAX_PERIOD].copy()  # :525
        aligned_in[TRAINING_OFFSET:] = inp[:FRAME_SIZE - TRAINING_OFFSET]  # :526
        # :527-537: pitch_mem[j] is aligned_in[i-1-j], so sum[i] = aligned_in[i]
        # + lpc[0]*aligned_in[i-1] + ... in j order, one add at a time
        ext = np.concatenate([self.pitch_mem[::-1], aligned_in]).astype(F)
        s = aligned_in.copy()
        for j in range(LPC_ORDER):
            s = (s + lpc[j] * ext[LPC_ORDER - 1 - j:LPC_ORDER - 1 - j + FRAME_SIZE]).astype(F)
        prev = np.concatenate([[self.pitch_filt], s[:-1]]).astype(F)
        self.exc_buf[PITCH_MAX_PERIOD:] = (s + F(.7) * prev).astype(F)  # :534
        self.pitch_filt = F(s[-1])
        self.pitch_mem = aligned_in[::-1][:LPC_ORDER].copy()
        # :539-576 cross-correlation on half-frames
        e = self.exc_buf
        for sub in range(2):
            off = sub * FRAME_SIZE // 2
            xcorr = np.zeros(PITCH_MAX_PERIOD, F)
            xa = np.ascontiguousarray(e[PITCH_MAX_PERIOD + off:PITCH_MAX_PERIOD + off + FRAME_SIZE // 2])
            ya = np.ascontiguousarray(e[off:off + FRAME_SIZE // 2 + PITCH_MAX_PERIOD])
            self.l.celt_pitch_xcorr(xa.ctypes.data, ya.ctypes.data, xcorr.ctypes.data, FRAME_SIZE // 2, PITCH_MAX_PERIOD)  # :542
            ener0 = _inner_prod(xa, xa)  # :543
            ener1 = float(_inner_prod(e[off:off + FRAME_SIZE // 2 - 1], e[off:off + FRAME_SIZE // 2 - 1]))  # :544, a double
            self.frame_weight[sub] = ener0  # :545
            row = np.zeros(PITCH_MAX_PERIOD, F)
            one_e0 = F(F(1) + ener0)
            for i in range(PITCH_MAX_PERIOD):  # :547-552
                a = e[i + off + FRAME_SIZE // 2 - 1]
                ener1 += float(F(a * a))
                ener = F(float(one_e0) + ener1)
                row[i] = F(F(F(2) * xcorr[i]) / ener)
                c = e[i + off]
                ener1 -= float(F(c * c))
            # :553-570 upsample by 3 and keep the max; reads the un-updated row
            interp = np.array([0.026184, -0.098339, 0.369938, 0.837891, -0.184969, 0.070242, -0.020947], F)
            idx = np.arange(4, PITCH_MAX_PERIOD - 4)
            val1 = np.zeros(len(idx), F)
            val2 = np.zeros(len(idx), F)
            for j in range(7):
                val1 = (val1 + row[idx - 3 + j] * interp[j]).astype(F)
                val2 = (val2 + row[idx + 3 - j] * interp[j]).astype(F)
            m = np.where(val1 > val2, val1, val2)
            new = row.copy()
            new[idx] = np.where(row[idx] > m, row[idx], m)
            self.xc[sub] = new

    # -- lpcnet_enc.c:814-870 ------------------------------------------------
    def process_single_frame(self):
        fw, xc, NS = self.frame_weight, self.xc, NSTATES
        fws = F(1e-15)
        for sub in range(2):
            fws = F(fws + fw[sub])  # :822
        for sub in range(2):
            fw[sub] = F(fw[sub] * F(F(2) / fws))  # :823
        pitch_prev = np.zeros((2, PITCH_MAX_PERIOD), np.int64)
        self.tied = []  # per half-frame: how many states share the maximum (tests: strict > matters)
        for sub in range(2):
            max_path_all = F(-1e15)
            best_i = 0
            r = xc[sub]
            for i in range(PITCH_MAX_PERIOD - 2 * PITCH_MIN_PERIOD):  # :827-830, serially
                h = _max16(_max16(r[(PITCH_MAX_PERIOD + i) // 2], r[(PITCH_MAX_PERIOD + i + 2) // 2]),
                           r[(PITCH_MAX_PERIOD + i - 1) // 2])
                if r[i] < F(h * F(1.1)):
                    r[i] = F(r[i] * F(.8))
            # :831-841 for every i, j ascending from max(-4, -i) while i+j < NS, strict >
            idx = np.arange(NS)
            max_prev = np.full(NS, F(self.pitch_max_path_all - F(6)), F)
            prev = np.full(NS, self.best_i, np.int64)
            for j in range(-4, 5):
                ok = (idx + j >= 0) & (idx + j < NS)
                pen = F(F(F(.02) * F(abs(j))) * F(abs(j)))
                v = np.full(NS, -np.inf, F)
                v[ok] = (self.pitch_max_path[0][idx[ok] + j] - pen).astype(F)
                up = ok & (v > max_prev)
                max_prev = np.where(up, v, max_prev).astype(F)
                prev = np.where(up, idx + j, prev)
            pitch_prev[sub, :NS] = prev
            self.pitch_max_path[1][:NS] = (max_prev + fw[sub] * r[:NS]).astype(F)  # :842
            for i in range(NS):  # :843-846
                if self.pitch_max_path[1][i] > max_path_all:
                    max_path_all = self.pitch_max_path[1][i]
                    best_i = i
            self.tied.append(int((self.pitch_max_path[1][:NS] == max_path_all).sum()))
            self.pitch_max_path[1][:NS] = (self.pitch_max_path[1][:NS] - max_path_all).astype(F)  # :849
            self.pitch_max_path[0] = self.pitch_max_path[1].copy()  # :852
            self.pitch_max_path_all = F(max_path_all)
            self.best_i = best_i
        best_i = self.best_i
        frame_corr = F(0)
        best = [0, 0]
        for sub in (1, 0):  # :859-863
            best[sub] = PITCH_MAX_PERIOD - best_i
            frame_corr = F(frame_corr + F(fw[sub] * xc[sub][best_i]))
            best_i = int(pitch_prev[sub][best_i])
        frame_corr = F(frame_corr / F(2))
        self.features[NB_BANDS] = F(F(.01) * F(max(66, min(510, best[0] + best[1])) - 200))  # :865
        self.features[NB_BANDS + 1] = F(frame_corr - F(.5))  # :866
        self.period = best[0] + best[1]  # twice the pitch period in samples at 16 kHz (two half-frames)

    def frame(self, pcm: np.ndarray) -> np.ndarray:
        """One frame as lpcnet_plc.c:251-254 runs it: pcm [160] int16 (or floats
        already converted) -> features [36]."""
        x = np.asarray(pcm).astype(F)
        assert x.shape == (FRAME_SIZE,)
        self.compute_frame_features(self.preemphasis(x))
        self.process_single_frame()
        return self.features.copy()


def run(pcm: np.ndarray) -> np.ndarray:
    """[nframes, 160] PCM of one stream from reset -> [nframes, 36] features."""
    r = EncRef()
    return np.stack([r.frame(f) for f in pcm])


def golden():
    """The committed fixture: pcm [5, 12, 160] int16, features [5, 12, 36] float32."""
    g = np.load(GOLDEN)
    return g["pcm"], g["features"]
