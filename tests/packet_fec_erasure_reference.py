"""RS(204,188) correction of packet-mode FEC frames with failed packet CRCs as erasures, from its definition: the section
"Erasures" of the contract at the top of include/dabgpu_packet_fec.h, read clause by clause into Python -- bytes, ints and
lists, no shared code with the headers, the kernels or dabgpu/synth.py.  The field arithmetic, the errors-only rule and the
frame finding are tests/packet_fec_reference.py's, the packet CRC is tests/packet_reference.py's; both are independent of
the headers.

    Suspect slots: steps 1 - 4 of the packet scan with fec non-zero, on each frame as received.
    Step 3 of a row: errata decoding by Sugiyama's Euclidean algorithm on the modified syndromes S(x) Gamma(x) mod x^16
    (the header's is Berlekamp-Massey on the syndromes above f), roots by evaluating the errata locator at every position,
    values by Forney -- and then the result is VERIFIED BY DEFINITION: the corrected row's 16 syndromes are recomputed, the
    differing positions counted inside and outside E, and anything but "a codeword that differs from the received row only in
    E and in e more positions, e = 0 or 2 e + f <= 14" leaves the row unchanged.  Every comparison is on bytes and integers.

    rx = Receiver(bitrate_kbps)
    out, counts = rx.call(frames)               # as packet_fec_reference.Receiver; counts: a RESULT_DTYPE record of 80 bytes
"""
import numpy as np

import packet_fec_reference as F
import packet_reference as R

EXTRA = ("slots_suspect", "frames_with_suspects", "frames_beyond_erasures", "rows_erasure_corrected", "erased_bytes_changed",
         "erasure_other_bytes_corrected")
COUNTERS = F.COUNTERS + EXTRA
RESULT_DTYPE = np.dtype([(n, np.int32) for n in F.COUNTERS] + [("reserved", np.int32)] + [(n, np.int32) for n in EXTRA] + [("reserved2", np.int32, (2,))])

#: alpha^(203 - c), the locator of codeword position c
X = [F.power(2, 203 - c) for c in range(204)]
#: 1 / a by a^254, tabulated once (INVERSE[0] is never read)
INVERSE = [0] + [F.inverse(a) for a in range(1, 256)]


def poly_divmod(a, b):
    """packet_fec_reference.poly_divmod with the tabulated inverse"""
    a, db = list(a), F.degree(b)
    q = [0] * max(1, len(a))
    inv = INVERSE[b[db]]
    for i in range(F.degree(a) - db, -1, -1):
        f = F.mul(a[i + db], inv)
        q[i] = f
        if f:
            for j in range(db + 1):
                a[i + j] ^= F.mul(f, b[j])
    return q, a


def suspect_slots(frame, S):
    """the scan of one logical frame (fec non-zero): which slots it counts as slots_bad"""
    frame = bytes(frame[:24 * S])
    bad, pos = [False] * S, 0
    while pos < S:
        p = frame[24 * pos:]
        L, addr = (p[0] >> 6) + 1, (p[0] & 3) << 8 | p[1]
        if addr == 1022 and L == 1:                                                   # 1: an FEC packet
            pos += 1
        elif pos + L > S:                                                             # 2
            bad[pos] = True
            pos += 1
        elif R.crc(p[:24 * L - 2]) != (p[24 * L - 2] << 8 | p[24 * L - 1]):           # 3
            bad[pos] = True
            pos += 1
        else:                                                                         # 4
            pos += L
    return bad


def errata_guess(s, E):
    """an errata pattern {position: value} from the 16 syndromes of one row and the erased columns, to be verified: not
    trusted.  Values may be zero."""
    f = len(E)
    gamma = [1]
    for c in E:
        gamma = F.poly_mul(gamma, [1, X[c]])
    t = F.poly_mul([int(v) for v in s], gamma)[:16]                        # the modified syndromes
    r0, r1 = [0] * 16 + [1], list(t)
    t0, t1 = [0], [1]
    while 2 * F.degree(r1) >= 16 + f:
        q, rem = poly_divmod(r0, r1)
        r0, r1 = r1, rem
        t0, t1 = t1, F.poly_add(t0, F.poly_mul(q, t1))
    if F.degree(t1) < 0 or t1[0] == 0:
        return {}
    inv = INVERSE[t1[0]]
    lam = [F.mul(c, inv) for c in t1[:F.degree(t1) + 1]]
    om = [F.mul(c, inv) for c in r1]
    psi = F.poly_mul(lam, gamma)
    deriv = [psi[i] if i % 2 else 0 for i in range(1, len(psi))]
    at = np.zeros(204, np.uint16)                                          # the errata locator at every position, by Horner
    for coef in reversed(psi):
        at = F.vmul(at, F.X_INVERSE) ^ np.uint16(coef)
    out = {}
    for c in np.nonzero(at == 0)[0]:
        xi = F.X_INVERSE[c]
        d = F.poly_eval(deriv, xi)
        if d == 0:
            return {}
        out[int(c)] = F.mul(F.mul(X[c], F.poly_eval(om, xi)), INVERSE[d])
    return out


def correct_rows(rows, E):
    """rows [n][204] uint8, E the erased columns of all of them -> (corrected rows, verdicts); a verdict is ("clean",),
    ("errors", k), ("erasures", changed in E, changed outside E) or ("unchanged",)"""
    rows = np.asarray(rows, np.uint8)
    out, old = F.correct_rows(rows)                                        # steps 1 and 2
    verdicts = [("clean",) if v == 0 else ("errors", v) if v > 0 else ("unchanged",) for v in old]
    f, inside = len(E), set(E)
    if not 2 <= f <= 16:
        return out, verdicts
    syn = F.syndromes(rows)
    tried, index = [], []
    for i, v in enumerate(verdicts):
        if v != ("unchanged",):
            continue
        row = rows[i].copy()
        for c, val in errata_guess(syn[i], E).items():
            row[c] ^= val
        tried.append(row)
        index.append(i)
    if tried:
        # verified by definition: the 16 syndromes of the corrected row, and the positions that differ, inside and outside E
        check = F.syndromes(np.stack(tried))
        for row, i, sy in zip(tried, index, check):
            differ = [c for c in range(204) if row[c] != rows[i][c]]
            e = sum(1 for c in differ if c not in inside)
            if sy.any() or not differ or (e >= 1 and 2 * e + f > 14):
                continue
            out[i] = row
            verdicts[i] = ("erasures", len(differ) - e, e)
    return out, verdicts


class Receiver(F.Receiver):
    def __init__(self, bitrate_kbps):
        super().__init__(bitrate_kbps)
        self.suspect = []                  # of every slot since the fresh start, as received

    def _correct(self, q, n):
        first = q - 102
        a = b"".join(bytes(self.slots[first + i]) for i in range(94))
        p = b"".join(bytes(self.slots[first + 94 + i][2:]) for i in range(9))
        rows = np.array([[a[12 * c + r] for c in range(188)] + [p[12 * j + r] for j in range(16)] for r in range(12)], np.uint8)
        E = [c for i in range(94) if self.suspect[first + i] for c in (2 * i, 2 * i + 1)]
        n["frames_with_suspects"] += len(E) >= 2
        n["frames_beyond_erasures"] += len(E) > 16
        fixed, verdicts = correct_rows(rows, E)
        for r, v in enumerate(verdicts):
            if v[0] == "clean":
                n["rows_clean"] += 1
                continue
            if v[0] == "unchanged":
                n["rows_uncorrectable"] += 1
                continue
            n["rows_corrected" if v[0] == "errors" else "rows_erasure_corrected"] += 1
            for c in range(204):
                if fixed[r, c] == rows[r, c]:
                    continue
                if v[0] == "errors":
                    n["bytes_corrected" if c < 188 else "parity_bytes_corrected"] += 1
                else:
                    n["erased_bytes_changed" if c in E else "erasure_other_bytes_corrected"] += 1
                if c < 188:
                    b = 12 * c + r
                    self.slots[first + b // 24][b % 24] = int(fixed[r, c])

    def call(self, frames):
        S, D = self.S, self.D
        n = dict.fromkeys(COUNTERS, 0)
        n["cifs"], n["slots"] = len(frames), len(frames) * S
        for frame in frames:
            frame = bytes(np.asarray(frame, np.uint8)[:24 * S])
            bad = suspect_slots(frame, S)                                  # the frame as received, before any correction
            n["slots_suspect"] += sum(bad)
            base = len(self.slots)
            self.suspect += bad
            for pos in range(S):                                           # (all of the frame's slots are known to _correct)
                self.slots.append(bytearray(frame[24 * pos:24 * pos + 24]))
                self.marks.append(F.mark(self.slots[-1]))
            for pos in range(S):
                q = base + pos
                n["marks"] += self.marks[q] is not None
                if sum(1 for i in range(9) if q - 8 + i >= 0 and self.marks[q - 8 + i] == i) < 7:
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
            data = F.PADDING_PACKET * S if k < 0 else b"".join(bytes(s) for s in self.slots[k * S:(k + 1) * S])
            out[f] = np.frombuffer(data, np.uint8)
        self.frames_seen += len(frames)
        rec = np.zeros(1, RESULT_DTYPE)
        for key in COUNTERS:
            rec[key] = n[key]
        return out, rec


def total(results):
    return {k: sum(int(r[k][0]) for r in results) for k in COUNTERS}
