"""RS(204,188) correction of packet-mode FEC frames from its definition: the contract at the top of
include/dabgpu_packet_fec.h (EN 300 401 clause 5.3.5), read clause by clause into Python -- bytes, ints and lists, no shared
code with the header, the kernels or dabgpu/synth.py.

    GF(2^8) is carry-less multiplication and reduction by x^8 + x^4 + x^3 + x^2 + 1: no exp / log table anywhere (mul on
    ints; vmul the same eight steps on numpy arrays, so that the syndromes of many rows are one Horner run).
    Decoding is Sugiyama's Euclidean algorithm (the header's is Berlekamp-Massey), roots by evaluating the locator at every
    position, values by Forney -- and then the result is VERIFIED BY DEFINITION: the corrected row's 16 syndromes are
    recomputed and the differing positions counted; anything but "a codeword, 1 to 8 positions away" leaves the row unchanged.
    Every comparison is on bytes and integers: exact.

    rx = Receiver(bitrate_kbps)                 # a fresh start; it is the state between calls
    out, counts = rx.call(frames)               # frames: [n] rows of at least 3 * bitrate bytes -> out [n][3 * bitrate] uint8
                                                # (delayed by delay(bitrate) frames), counts: a RESULT_DTYPE record
"""
import numpy as np

COUNTERS = ("cifs", "slots", "marks", "frames", "frames_cut", "frames_overlapping", "rows_clean", "rows_corrected",
            "rows_uncorrectable", "bytes_corrected", "parity_bytes_corrected")
RESULT_DTYPE = np.dtype([(n, np.int32) for n in COUNTERS] + [("reserved", np.int32)])
POLY = 0x11D


def mul(a, b):
    """a(x) b(x) mod x^8 + x^4 + x^3 + x^2 + 1"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a & 0x100:
            a ^= POLY
    return r


def vmul(a, b):
    """mul on numpy arrays (uint16), element by element"""
    a, b = np.asarray(a, np.uint16).copy(), np.asarray(b, np.uint16).copy()
    a, b = np.broadcast_arrays(a, b)
    a, b = a.copy(), b.copy()
    r = np.zeros(a.shape, np.uint16)
    for _ in range(8):
        r ^= np.where(b & 1, a, 0).astype(np.uint16)
        b >>= 1
        a <<= 1
        a ^= np.where(a & 0x100, POLY, 0).astype(np.uint16)
    return r


def power(a, n):
    r = 1
    for _ in range(n):
        r = mul(r, a)
    return r


def inverse(a):
    assert a
    return power(a, 254)


#: alpha^k for the 16 roots of the generator, and alpha^-(203 - c) for the 204 positions (by repeated multiplication)
ROOTS = [power(2, k) for k in range(16)]
X_INVERSE = [inverse(power(2, 203 - c)) for c in range(204)]


def syndromes(rows):
    """rows [n][204] -> [n][16]: S_k = sum_c cw[c] alpha^(k (203 - c)), by Horner from cw[0], the coefficient of x^203"""
    rows = np.asarray(rows, np.uint16)
    s = np.zeros((rows.shape[0], 16), np.uint16)
    roots = np.array(ROOTS, np.uint16)[None, :]
    for c in range(204):
        s = vmul(s, roots) ^ rows[:, c:c + 1]
    return s


def poly_eval(p, x):
    """p[i] the coefficient of x^i"""
    r = 0
    for coef in reversed(p):
        r = mul(r, x) ^ coef
    return r


def degree(p):
    d = len(p) - 1
    while d >= 0 and p[d] == 0:
        d -= 1
    return d


def poly_divmod(a, b):
    a, db = list(a), degree(b)
    q = [0] * max(1, len(a))
    inv = inverse(b[db])
    for i in range(degree(a) - db, -1, -1):
        f = mul(a[i + db], inv)
        q[i] = f
        if f:
            for j in range(db + 1):
                a[i + j] ^= mul(f, b[j])
    return q, a


def poly_mul(a, b):
    r = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                r[i + j] ^= mul(x, y)
    return r


def poly_add(a, b):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else 0) ^ (b[i] if i < len(b) else 0) for i in range(n)]


def euclid(s):
    """Sugiyama: x^16 and S(x) divided until the remainder's degree is below 8 -> (locator, evaluator), or None"""
    r0, r1 = [0] * 16 + [1], list(s)
    t0, t1 = [0], [1]
    while degree(r1) >= 8:
        q, rem = poly_divmod(r0, r1)
        r0, r1 = r1, rem
        t0, t1 = t1, poly_add(t0, poly_mul(q, t1))
    if degree(t1) < 0 or t1[0] == 0:
        return None
    inv = inverse(t1[0])
    return [mul(c, inv) for c in t1[:degree(t1) + 1]], [mul(c, inv) for c in r1]


def guess(s):
    """an error pattern {position: value} from the syndromes of one row, to be verified: not trusted"""
    le = euclid([int(v) for v in s])
    if le is None:
        return {}
    lam, om = le
    deriv = [lam[i] if i % 2 else 0 for i in range(1, len(lam))]           # d/dx in characteristic 2
    at = np.zeros(204, np.uint16)                                          # the locator at every position, by Horner
    for coef in reversed(lam):
        at = vmul(at, X_INVERSE) ^ np.uint16(coef)
    out = {}
    for c in np.nonzero(at == 0)[0]:
        xi = X_INVERSE[c]
        d = poly_eval(deriv, xi)
        if d == 0:
            return {}
        out[int(c)] = mul(mul(inverse(xi), poly_eval(om, xi)), inverse(d))
    return out


def correct_rows(rows):
    """rows [n][204] uint8 -> (corrected rows, verdicts): 0 a codeword, k > 0 a codeword k <= 8 positions away was found and
    taken, -1 unchanged"""
    rows = np.asarray(rows, np.uint8)
    out, verdicts = rows.copy(), []
    syn = syndromes(rows)
    tried, index = [], []
    for i in range(len(rows)):
        if not syn[i].any():
            verdicts.append(0)
            continue
        verdicts.append(-1)
        pattern = guess(syn[i])
        if 1 <= len(pattern) <= 8 and all(pattern.values()):
            row = rows[i].copy()
            for c, v in pattern.items():
                row[c] ^= v
            tried.append(row)
            index.append(i)
    if tried:
        # verified by definition: the 16 syndromes of the corrected row, and the positions that differ
        check = syndromes(np.stack(tried))
        for row, i, s in zip(tried, index, check):
            differ = int((row != rows[i]).sum())
            if not s.any() and 1 <= differ <= 8:
                out[i] = row
                verdicts[i] = differ
    return out, verdicts


def delay(bitrate_kbps):
    return -(-102 // (bitrate_kbps // 8))


def crc(data):
    """x^16 + x^12 + x^5 + 1, register all ones, complemented, bit by bit"""
    reg = 0xFFFF
    for byte in data:
        for bit in range(7, -1, -1):
            top = (reg >> 15) & 1
            reg = (reg << 1) & 0xFFFF
            if top ^ ((byte >> bit) & 1):
                reg ^= 0x1021
    return reg ^ 0xFFFF


_PAD = bytes([0x0C, 0, 0]) + bytes(19)
PADDING_PACKET = _PAD + crc(_PAD).to_bytes(2, "big")


def mark(slot):
    h0, h1 = int(slot[0]), int(slot[1])
    c = (h0 >> 2) & 15
    return c if (h0 >> 6) == 0 and ((h0 & 3) << 8 | h1) == 1022 and c <= 8 else None


class Receiver:
    def __init__(self, bitrate_kbps):
        self.S = bitrate_kbps // 8
        self.D = delay(bitrate_kbps)
        self.marks = []                    # of every slot since the fresh start, as received
        self.slots = []                    # every slot since the fresh start: bytearrays, corrected in place
        self.frames_seen = 0
        self.last_end = -1

    def _frame_ends_at(self, q):
        return sum(1 for i in range(9) if q - 8 + i >= 0 and self.marks[q - 8 + i] == i) >= 7

    def _correct(self, q, n):
        first = q - 102
        a = b"".join(bytes(self.slots[first + i]) for i in range(94))
        p = b"".join(bytes(self.slots[first + 94 + i][2:]) for i in range(9))
        rows = np.array([[a[12 * c + r] for c in range(188)] + [p[12 * j + r] for j in range(16)] for r in range(12)], np.uint8)
        fixed, verdicts = correct_rows(rows)
        for r, v in enumerate(verdicts):
            if v == 0:
                n["rows_clean"] += 1
            elif v < 0:
                n["rows_uncorrectable"] += 1
            else:
                n["rows_corrected"] += 1
                for c in range(204):
                    if fixed[r, c] != rows[r, c]:
                        n["bytes_corrected" if c < 188 else "parity_bytes_corrected"] += 1
                        if c < 188:
                            b = 12 * c + r
                            self.slots[first + b // 24][b % 24] = int(fixed[r, c])

    def call(self, frames):
        S, D = self.S, self.D
        n = dict.fromkeys(COUNTERS, 0)
        n["cifs"], n["slots"] = len(frames), len(frames) * S
        for frame in frames:
            frame = bytes(np.asarray(frame, np.uint8)[:24 * S])
            for pos in range(S):
                slot = bytearray(frame[24 * pos:24 * pos + 24])
                self.slots.append(slot)
                self.marks.append(mark(slot))
                n["marks"] += self.marks[-1] is not None
                q = len(self.slots) - 1
                if not self._frame_ends_at(q):
                    continue
                if q - 102 < 0:
                    n["frames_cut"] += 1
                elif q - 102 <= self.last_end:
                    n["frames_overlapping"] += 1
                else:
                    n["frames"] += 1
                    self.last_end = q
                    self._correct(q, n)
        out = np.zeros((len(frames), 24 * S), np.uint8)
        for f in range(len(frames)):
            k = self.frames_seen + f - D
            data = PADDING_PACKET * S if k < 0 else b"".join(bytes(s) for s in self.slots[k * S:(k + 1) * S])
            out[f] = np.frombuffer(data, np.uint8)
        self.frames_seen += len(frames)
        rec = np.zeros(1, RESULT_DTYPE)
        for key in COUNTERS:
            rec[key] = n[key]
        return out, rec


def total(results):
    return {k: sum(int(r[k][0]) for r in results) for k in COUNTERS}
