"""CPU reference of the 1.6 kb/s encoder (lpcnet_encode, quantize = encode =
1, and lpcnet_compute_features, quantize = encode = 0; lpcnet_enc.c:53-400,
498-577, 579-743, 872-909, and perform_double_interp, common.c:36-65) for one
stream, in float32 numpy.  Builds on enc_ref.EncRef (preemphasis and
compute_frame_features around the reference's own compiled freq.c / pitch.c)
and restates the pcount-indexed rows, process_superframe, the quantisers with
their literal survivor merge, the bit packer and the x86 (int) cast.
lpcnet_enc.c itself cannot be compiled (nnet_data.h and ceps_codebooks.c are
generated and absent); tests/test_encode_ref.py checks this restatement against
the decoder oracle.  Shared by tests/test_encode_ref.py,
tests/test_gpu_encode.py and tests/golden/make_enc_packet_golden.py.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import math
import os

import numpy as np

import enc_ref as E

F = np.float32
NB = E.NB_BANDS
NB1 = NB - 1
PMAX, PMIN, NS = E.PITCH_MAX_PERIOD, E.PITCH_MIN_PERIOD, E.NSTATES
SURVIVORS = 5
FORBIDDEN_INTERP = 7
INT_MIN = -2 ** 31
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enc_packets.npz")
NPACKETS = 6
FIELDS = ["c0_id", "main_pitch", "modulation", "corr_id", "vq_end0", "vq_end1", "vq_end2", "vq_mid", "interp_id"]
FIELD_BITS = [7, 6, 3, 2, 10, 10, 10, 13, 3]


def cvtt(v: float) -> int:
    """(int) of a double as x86's cvttsd2si: NaN, infinities and out-of-range
    values give INT_MIN."""
    if v != v or v in (math.inf, -math.inf) or not (-2147483649.0 < v < 2147483648.0):
        return INT_MIN
    return int(v)


def dfloor(v: float) -> float:
    return v if (v != v or v in (math.inf, -math.inf)) else float(math.floor(v))


def dlog(v: float) -> float:
    """The host's double log with C's results at and below zero."""
    if v != v or v < 0:
        return math.nan
    if v == 0:
        return -math.inf
    return math.log(v)


def main_pitch_of(center_pitch) -> int:
    """lpcnet_enc.c:678-679."""
    with np.errstate(all="ignore"):
        q = float(F(center_pitch) / F(PMIN))
    m = cvtt(dfloor(.5 + 21. * 1.442695041 * dlog(q)))
    return max(0, min(63, m))


def _max16(a, b):
    return a if a > b else b  # arch.h:73


def _min16(a, b):
    return a if a < b else b  # arch.h:72


def split_codebooks(cb: dict):
    return (cb["ceps_codebook1"].reshape(1024, NB1), cb["ceps_codebook2"].reshape(1024, NB1),
            cb["ceps_codebook3"].reshape(1024, NB1), cb["ceps_codebook_diff4"].reshape(4096, NB))


def blob_codebooks(blob: bytes) -> dict:
    off, out = 0, {}
    while off < len(blob):
        size, block = np.frombuffer(blob[off + 12:off + 20], np.int32)
        name = blob[off + 20:off + 64].split(b"\0")[0].decode()
        if name.startswith("ceps_codebook"):
            out[name] = np.frombuffer(blob[off + 64:off + 64 + int(size)], np.float32)
        off += 64 + int(block)
    return out


def distances(codebook: np.ndarray, x: np.ndarray, sign: float = -1.0) -> np.ndarray:
    """d += (x[j]-c[j])*(x[j]-c[j]) in j order, for every entry (x [ndim] or [n, ndim])."""
    d = np.zeros(codebook.shape[0], F)
    for j in range(codebook.shape[1]):
        xj = x[..., j]
        t = (xj - codebook[:, j]).astype(F) if sign < 0 else (xj + codebook[:, j]).astype(F)
        d = (d + (t * t).astype(F)).astype(F)
    return d


def vq_quantize_mbest(codebook, x, mbest=SURVIVORS):
    """lpcnet_enc.c:53-78, literally."""
    d_all = distances(codebook, x)
    dist = [F(1e15)] * mbest
    index = [0] * mbest
    for i in range(len(d_all)):
        d = d_all[i]
        if d < dist[mbest - 1]:
            pos = mbest - 1
            for j in range(mbest - 1):
                if d < dist[j]:
                    pos = j
                    break
            for j in range(mbest - 1, pos, -1):
                dist[j] = dist[j - 1]
                index[j] = index[j - 1]
            dist[pos] = d
            index[pos] = int(i)
    return dist, index


def quantize_3stage_mbest(cbs, x: np.ndarray):
    """lpcnet_enc.c:133-241.  x [17] is replaced by its quantised value;
    returns (entry[3], the first stage's nearest entry)."""
    c1, c2, c3 = cbs[:3]
    curr_dist, curr_index = vq_quantize_mbest(c1, x)
    index1 = [[curr_index[k], 0, 0] for k in range(SURVIVORS)]
    index2 = [[0, 0, 0] for _ in range(SURVIVORS)]
    index3 = [[0, 0, 0] for _ in range(SURVIVORS)]
    glob_dist = [F(0)] * SURVIVORS

    def stage(k, prev, cur, depth, curr_dist, curr_index):
        if k == 0:
            for m in range(SURVIVORS):
                cur[m][:depth] = prev[k][:depth]
                cur[m][depth] = curr_index[m]
                glob_dist[m] = curr_dist[m]
        elif curr_dist[0] < glob_dist[SURVIVORS - 1]:
            m = 0
            for pos in range(SURVIVORS):
                if curr_dist[m] < glob_dist[pos]:  # m advances only on insertion
                    for j in range(SURVIVORS - 1, pos, -1):
                        glob_dist[j] = glob_dist[j - 1]
                        cur[j][:depth + 1] = cur[j - 1][:depth + 1]
                    glob_dist[pos] = curr_dist[m]
                    cur[pos][:depth] = prev[k][:depth]
                    cur[pos][depth] = curr_index[m]
                    m += 1

    for k in range(SURVIVORS):
        diff = (x - c1[index1[k][0]]).astype(F)
        cd, ci = vq_quantize_mbest(c2, diff)
        stage(k, index1, index2, 1, cd, ci)
    for k in range(SURVIVORS):
        diff = ((x - c1[index2[k][0]]).astype(F) - c2[index2[k][1]]).astype(F)
        cd, ci = vq_quantize_mbest(c3, diff)
        stage(k, index2, index3, 2, cd, ci)
    e = index3[0]
    x[:] = ((c1[e[0]] + c2[e[1]]).astype(F) + c3[e[2]]).astype(F)
    return list(e), index1[0][0]


def find_nearest_multi(codebook, x4: np.ndarray, sign: int) -> int:
    """lpcnet_enc.c:243-280: x4 [4, ndim], entry i against x4[i & 3]."""
    n = codebook.shape[0]
    xi = x4[np.arange(n) & 3]
    min_dist, nearest = F(1e15), 0
    d = distances(codebook, xi)
    i = int(np.argmin(d))  # the first minimum, as the strict < keeps it
    if d[i] < min_dist:
        min_dist, nearest = d[i], i
    if sign:
        d = distances(codebook, xi, +1.0)
        i = int(np.argmin(d))
        if d[i] < min_dist:
            min_dist, nearest = d[i], i + n
    return nearest


def preds4(left, right):
    h = (F(.5) * (left + right).astype(F)).astype(F)
    return np.stack([h, h, left, right]).astype(F)


def quantize_diff(x, left, right, codebook, bits=12, sign=1) -> int:
    """lpcnet_enc.c:283-318; x [18] replaced.  Returns *entry."""
    pred = preds4(left, right)
    target = (x[None, :] - pred).astype(F)
    entry = find_nearest_multi(codebook, target, sign)
    idn, s = entry, F(1)
    if idn >= 1 << bits:
        s = F(-1)
        idn -= 1 << bits
    x[:] = (pred[idn & 3] + (s * codebook[idn]).astype(F)).astype(F)
    return entry


def interp_search(x, left, right):
    """lpcnet_enc.c:320-340: dist_out[3] (best_pred is not used by the caller)."""
    pred = preds4(left, right)
    out = []
    for k in range(1, 4):
        d = F(0)
        for i in range(NB):
            t = F(x[i] - pred[k][i])
            d = F(d + F(t * t))
        out.append(d)
    return out


def double_interp_search(f, mem) -> int:
    """lpcnet_enc.c:379-400."""
    d0 = interp_search(f[0][:NB], mem, f[1][:NB])
    d1 = interp_search(f[2][:NB], f[1][:NB], f[3][:NB])
    best_id, min_dist = 0, F(1e15)
    for i in range(3):
        for j in range(3):
            idn = 3 * i + j
            d = F(d0[i] + d1[j])
            if d < min_dist and idn != FORBIDDEN_INTERP:
                min_dist, best_id = d, idn
    return best_id - (best_id >= FORBIDDEN_INTERP)


def perform_double_interp(f, mem, best_id):
    """common.c:36-65."""
    best_id += best_id >= FORBIDDEN_INTERP
    id0, id1 = best_id // 3, best_id % 3
    p = lambda l, r: [(F(.5) * (l + r).astype(F)).astype(F), l.copy(), r.copy()]  # noqa: E731
    f[0][:NB] = p(mem, f[1][:NB])[id0]
    f[2][:NB] = p(f[1][:NB], f[3][:NB])[id1]


def bits_pack(fields) -> bytes:
    """lpcnet_enc.c:435-463: MSB first, the low nb_bits of each field."""
    bits = ""
    for v, n in zip(fields, FIELD_BITS):
        for b in range(n - 1, -1, -1):
            bits += str((v >> b) & 1)
    assert len(bits) == 64
    return bytes(int(bits[8 * k:8 * k + 8], 2) for k in range(8))


def unpack(packet) -> dict:
    bits = "".join(format(b, "08b") for b in bytes(packet))
    out, pos = {}, 0
    for name, n in zip(FIELDS, FIELD_BITS):
        out[name] = int(bits[pos:pos + n], 2)
        pos += n
    return out


class EncPacketRef(E.EncRef):
    """One LPCNetEncState: EncRef's single-frame path (frame()) and the
    four-frame calls on the same state."""

    def __init__(self, codebooks=None):
        self.cbs = None if codebooks is None else split_codebooks(codebooks)
        super().__init__()

    def reset(self):
        super().reset()
        self.xc8 = np.zeros((8, PMAX), F)          # xc[2..9]; xc[0..1] are written, never read
        self.fw8 = np.zeros(8, F)                  # frame_weight[2..9]
        self.feat4 = np.zeros((4, E.NB_TOTAL_FEATURES), F)
        self.vq_mem = np.zeros(NB, F)
        self.info = {}

    def state_bytes(self) -> bytes:
        """The layout of lpcnet_batch_encode_save_state."""
        return super().state_bytes() + self.vq_mem.tobytes()

    def _analyse(self, pcm640):
        pcm = np.asarray(pcm640).reshape(4, E.FRAME_SIZE)
        for k in range(4):  # :884-890, pcount = k
            self.compute_frame_features(self.preemphasis(pcm[k].astype(F)))
            self.xc8[2 * k:2 * k + 2] = self.xc
            self.fw8[2 * k:2 * k + 2] = self.frame_weight
            self.feat4[k] = self.features

    def process_superframe(self, quantize: bool):
        """lpcnet_enc.c:579-743; returns the packet (quantize = encode = 1) or None."""
        fw, xc = self.fw8, self.xc8
        s = F(1e-15)
        for sub in range(8):
            s = F(s + fw[sub])
        with np.errstate(all="ignore"):
            for sub in range(8):
                fw[sub] = F(fw[sub] * F(F(8) / s))
        pitch_prev = np.zeros((8, PMAX), np.int64)
        for sub in range(8):
            max_path_all, best_i = F(-1e15), 0
            r = xc[sub]
            for i in range(PMAX - 2 * PMIN):
                h = _max16(_max16(r[(PMAX + i) // 2], r[(PMAX + i + 2) // 2]), r[(PMAX + i - 1) // 2])
                if r[i] < F(h * F(1.1)):
                    r[i] = F(r[i] * F(.8))
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
            self.pitch_max_path[1][:NS] = (max_prev + (fw[sub] * r[:NS]).astype(F)).astype(F)
            for i in range(NS):
                if self.pitch_max_path[1][i] > max_path_all:
                    max_path_all, best_i = self.pitch_max_path[1][i], i
            self.pitch_max_path[1][:NS] = (self.pitch_max_path[1][:NS] - max_path_all).astype(F)
            self.pitch_max_path[0] = self.pitch_max_path[1].copy()
            self.pitch_max_path_all = F(max_path_all)
            self.best_i = best_i
        best_i = self.best_i
        frame_corr = F(0)
        best = [0] * 10
        for sub in range(7, -1, -1):
            best[2 + sub] = PMAX - best_i
            frame_corr = F(frame_corr + F(fw[sub] * xc[sub][best_i]))
            best_i = int(pitch_prev[sub][best_i])
        frame_corr = F(frame_corr / F(8))
        if quantize and frame_corr < 0:
            frame_corr = F(0)
        sx = sxx = sxy = sy = sw = F(0)
        for sub in range(2, 10):
            w = fw[sub - 2]
            sw = F(sw + w)
            sx = F(sx + F(w * F(sub)))
            sxx = F(sxx + F(F(w * F(sub)) * F(sub)))
            sxy = F(sxy + F(F(w * F(sub)) * F(best[sub])))
            sy = F(sy + F(w * F(best[sub])))
        voiced = float(frame_corr) >= .3
        with np.errstate(all="ignore"):
            best_a = F(F(F(sw * sxy) - F(sx * sy)) / F(F(sw * sxx) - F(sx * sx)))
            if voiced:
                mean_pitch = F(sy / sw)
                max_a = F(mean_pitch / F(32))
                best_a = _min16(max_a, _max16(F(-max_a), best_a))
                corr_id = cvtt(dfloor(float(F(F(frame_corr - F(.3)) / F(.175)))))
                if quantize:
                    frame_corr = F(F(0.3875) + F(F(.175) * F(corr_id)))
            else:
                best_a = F(0)
                corr_id = cvtt(dfloor(float(F(frame_corr / F(.075)))))
                if quantize:
                    frame_corr = F(F(0.0375) + F(F(.075) * F(corr_id)))
            best_b = F(F(sy - F(best_a * sx)) / sw)
            center_pitch = F(best_b + F(F(5.5) * best_a))
            main_pitch = main_pitch_of(center_pitch)
            modulation = cvtt(dfloor(.5 + float(F(F(F(16 * 7) * best_a) / center_pitch))))
        modulation = max(-3, min(3, modulation))
        f = self.feat4
        for sub in range(4):
            if quantize:
                p = F(math.pow(2.0, main_pitch / 21.) * PMIN)
                p = F(p * F(F(1) + F(F(F(F(modulation) / F(16)) / F(7)) * F(2 * sub - 3))))
                p = _min16(F(255), _max16(F(33), p))
                f[sub][NB] = F(F(.02) * F(p - F(100)))
            else:
                f[sub][NB] = F(F(.01) * F(max(66, min(510, best[2 + 2 * sub] + best[2 + 2 * sub + 1])) - 200))
            f[sub][NB + 1] = F(frame_corr - F(.5))
        c0_id, vq_end, vq_mid, interp_id, nearest1 = 0, [0, 0, 0], 0, 0, 0
        if quantize:
            c0_id = cvtt(dfloor(.5 + float(F(f[3][0] * F(4)))))
            c0_id = max(-64, min(63, c0_id))
            f[3][0] = F(F(c0_id) / F(4))
            x = f[3][1:NB].copy()
            vq_end, nearest1 = quantize_3stage_mbest(self.cbs, x)
            f[3][1:NB] = x
            x = f[1][:NB].copy()
            vq_mid = quantize_diff(x, self.vq_mem, f[3][:NB].copy(), self.cbs[3])
            f[1][:NB] = x
            interp_id = double_interp_search(f, self.vq_mem)
            perform_double_interp(f, self.vq_mem, interp_id)
        for sub in range(4):  # :714-717
            lpc = np.zeros(E.LPC_ORDER, F)
            ceps = np.ascontiguousarray(f[sub][:NB])
            self.l.lpc_from_cepstrum(lpc.ctypes.data, ceps.ctypes.data)
            f[sub][NB + 2:] = lpc
        self.vq_mem = f[3][:NB].copy()
        self.info = dict(voiced=bool(voiced), modulation=modulation, main_pitch=main_pitch, corr_id=corr_id, c0_id=c0_id,
                         vq_end=vq_end, vq_mid=vq_mid, interp_id=interp_id, nearest1=nearest1)
        if not quantize:
            return None
        return bits_pack([c0_id + 64, main_pitch, modulation + 4 if voiced else 0, corr_id, vq_end[0], vq_end[1], vq_end[2],
                          vq_mid, interp_id])

    def encode(self, pcm640) -> tuple[bytes, np.ndarray]:
        """lpcnet_encode: pcm [640] int16 -> (packet, st->features [4, 36])."""
        self._analyse(pcm640)
        pk = self.process_superframe(True)
        return pk, self.feat4.copy()

    def compute_features4(self, pcm640) -> np.ndarray:
        """lpcnet_compute_features: pcm [640] int16 -> features [4, 36]."""
        self._analyse(pcm640)
        self.process_superframe(False)
        return self.feat4.copy()


def tie_codebooks(cb: dict) -> dict:
    """Entry i + 512 of every stage equals entry i, entry i + 2048 of the
    difference codebook equals entry i; the second stage and the difference
    codebook also hold an all-zero row pair (for the latter both signs tie as
    well)."""
    c = {k: v.copy() for k, v in cb.items()}
    for k in ("ceps_codebook1", "ceps_codebook2", "ceps_codebook3"):
        a = c[k].reshape(1024, 17)
        a[512:] = a[:512]
    c["ceps_codebook2"].reshape(1024, 17)[[7, 519]] = 0
    d = c["ceps_codebook_diff4"].reshape(4096, 18)
    d[2048:] = d[:2048]
    d[[5, 2053]] = 0
    return c


# -- the fixture ----------------------------------------------------------------

_fix = None


def fixture() -> dict:
    """The committed fixture, read-only (tests/golden/make_enc_packet_golden.py
    lists its arrays)."""
    global _fix
    if _fix is None:
        with np.load(GOLDEN) as g:
            _fix = {k: g[k] for k in g.files}
        for v in _fix.values():
            v.setflags(write=False)
    return _fix


def fixture_codebooks(prefix: str = "cb") -> dict:
    fx = fixture()
    return {"ceps_codebook1": fx[prefix + "1"], "ceps_codebook2": fx[prefix + "2"], "ceps_codebook3": fx[prefix + "3"],
            "ceps_codebook_diff4": fx[prefix + "d"]}
