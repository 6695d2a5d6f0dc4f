"""DAB+ super-frame checks restated from their definitions (ETSI TS 102 563 clauses 5.2 and 6): a test helper, written
without any table or code of oracle/ or dabgpu/synth.py, so that a mistake those share with the HIP kernel cannot pass.

- GF(2^8) with P(x) = x^8+x^4+x^3+x^2+1 and alpha = 2, its tables made here from bitwise multiplication.
- RS(120,110): shortened from RS(255,245), generator prod_{k=0..9} (x + alpha^k); byte i of a codeword is the coefficient
  of x^(119 - i).  The parity-check matrix is H[k][i] = alpha^(k (119 - i)).
- The decoder is Peterson-Gorenstein-Zierler: largest nonsingular syndrome matrix, locator roots by trying every
  position, error values by a second elimination, and a final check that the result is a codeword.  It returns the
  unique codeword within distance 5 of its input, or None when there is none -- what a bounded-distance decoder must do.
- Fire code: remainder of m(x) x^16 by G(x) = (x^11 + 1)(x^5 + x^3 + x^2 + x + 1), by plain division over GF(2).
- AU CRC: CRC16-CCITT, register started at 0xFFFF, inverted (binascii.crc_hqx).
"""
import binascii

import numpy as np

N, K, NPAR, T = 120, 110, 10, 5

# status record of one super-frame, the layout of dabgpu_superframe_status
STATUS_DTYPE = np.dtype([("firecode_ok", np.int32), ("rs_corrected", np.int32), ("rs_uncorrectable", np.int32),
                         ("num_aus", np.int32), ("au_crc_mask", np.int32), ("au_start", np.int32, (8,)),
                         ("reserved", np.int32, (3,))])


# ------------------------------------------------------------------------------------------------------------ GF(2^8)
def gf_mul_bits(a, b):
    """a b in GF(2^8) / x^8+x^4+x^3+x^2+1, by shift and add."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11D
        b >>= 1
    return r


def _tables():
    exp = np.zeros(255, np.int64)
    log = np.full(256, -1, np.int64)
    x = 1
    for i in range(255):
        exp[i] = x
        log[x] = i
        x = gf_mul_bits(x, 2)
    assert x == 1 and (log[1:] >= 0).all(), "alpha = 2 must generate the multiplicative group"
    return exp, log


EXP, LOG = _tables()


def gmul(a, b):
    return 0 if a == 0 or b == 0 else int(EXP[(LOG[a] + LOG[b]) % 255])


def ginv(a):
    return int(EXP[(255 - LOG[a]) % 255])


def gpow(p):
    """alpha^p for any integer p."""
    return int(EXP[p % 255])


def gmul_vec(a, b):
    """elementwise a b of integer arrays (broadcast)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    r = EXP[(LOG[a] + LOG[b]) % 255]
    return np.where((a == 0) | (b == 0), 0, r)


def gf_solve(A, b):
    """x with A x = b over GF(2^8) (A square, lists of ints), or None when A is singular."""
    n = len(A)
    M = [list(map(int, A[i])) + [int(b[i])] for i in range(n)]
    for c in range(n):
        piv = next((r for r in range(c, n) if M[r][c]), None)
        if piv is None:
            return None
        M[c], M[piv] = M[piv], M[c]
        inv = ginv(M[c][c])
        M[c] = [gmul(inv, v) for v in M[c]]
        for r in range(n):
            if r != c and M[r][c]:
                f = M[r][c]
                M[r] = [v ^ gmul(f, w) for v, w in zip(M[r], M[c])]
    return [M[i][n] for i in range(n)]


# --------------------------------------------------------------------------------------------------------- RS(120,110)
# H[k][i] = alpha^(k (119 - i)): r is a codeword iff H r = 0
H = np.array([[gpow(k * (N - 1 - i)) for i in range(N)] for k in range(NPAR)], np.int64)


def syndromes(words):
    """S_k = r(alpha^k), k = 0..9, first byte the highest power: [..., 120] -> [..., 10] (int64)."""
    w = np.asarray(words, np.int64)
    shape = w.shape[:-1]
    w = w.reshape(-1, N)
    out = np.zeros((w.shape[0], NPAR), np.int64)
    for c0 in range(0, w.shape[0], 2048):
        blk = w[c0:c0 + 2048]
        terms = gmul_vec(blk[:, None, :], H[None, :, :])             # [rows][k][i]
        out[c0:c0 + 2048] = np.bitwise_xor.reduce(terms, axis=2)
    return out.reshape(shape + (NPAR,))


def _parity_map():
    """P [10][110] with parity = P data: from H_par parity = H_data data (any 10 columns of H are independent)."""
    hp = H[:, K:].tolist()
    P = np.zeros((NPAR, K), np.int64)
    for i in range(K):
        P[:, i] = gf_solve(hp, H[:, i].tolist())
    return P


_P = _parity_map()


def rs_encode(data):
    """[..., 110] data bytes -> [..., 120] systematic codewords (uint8)."""
    d = np.asarray(data, np.int64)
    shape = d.shape[:-1]
    d = d.reshape(-1, K)
    par = np.zeros((d.shape[0], NPAR), np.int64)
    for c0 in range(0, d.shape[0], 4096):
        blk = d[c0:c0 + 4096]
        par[c0:c0 + 4096] = np.bitwise_xor.reduce(gmul_vec(blk[:, None, :], _P[None, :, :]), axis=2)
    return np.concatenate([d, par], axis=1).astype(np.uint8).reshape(shape + (N,))


def rs_decode(word):
    """Bounded-distance decode of one 120-byte column: (codeword uint8[120], number of corrected bytes), or None when no
    codeword lies within distance 5."""
    r = np.asarray(word, np.uint8)
    S = [int(v) for v in syndromes(r)]
    if not any(S):
        return r.copy(), 0
    for nu in range(T, 0, -1):
        # Newton: sum_{m=0..nu} Lambda_m S_{j+nu-m} = 0 for j = 0..nu-1
        A = [[S[j + nu - m] for m in range(1, nu + 1)] for j in range(nu)]
        lam = gf_solve(A, [S[j + nu] for j in range(nu)])
        if lam is not None:
            break
    else:
        return None
    lam = [1] + lam
    # roots X^-1 of Lambda, X = alpha^p; p = 119 - i for byte i, p = 120..254 are the shortened (always zero) bytes
    p = np.arange(255)
    v = np.zeros(255, np.int64)
    for m, c in enumerate(lam):
        v ^= gmul_vec(c, EXP[(-p * m) % 255])
    roots = [int(x) for x in np.flatnonzero(v == 0)]
    if len(roots) != nu or max(roots) >= N:
        return None
    # error values: sum_l e_l X_l^k = S_k, k = 0..nu-1
    e = gf_solve([[gpow(k * p) for p in roots] for k in range(nu)], S[:nu])
    if e is None or not all(e):
        return None
    c = r.copy()
    for p, v in zip(roots, e):
        c[N - 1 - p] ^= v
    if syndromes(c).any():                                           # Lambda from fewer than 10 syndromes: check them all
        return None
    return c, nu


def min_weight_codeword(support, rng=None):
    """The codeword (uint8[120]) of weight 11 on the given 11 positions: H[:, support] x = 0 with x_0 = 1 (MDS: unique up to
    scale, every x_i non-zero), scaled by a random non-zero byte when rng is given."""
    support = [int(i) for i in support]
    assert len(set(support)) == NPAR + 1 and all(0 <= i < N for i in support)
    rest = gf_solve([[int(H[k, i]) for i in support[1:]] for k in range(NPAR)], [int(H[k, support[0]]) for k in range(NPAR)])
    x = [1] + rest
    scale = 1 if rng is None else int(rng.integers(1, 256))
    c = np.zeros(N, np.uint8)
    for i, v in zip(support, x):
        assert v != 0
        c[i] = gmul(v, scale)
    assert not syndromes(c).any()
    return c


def forced_miscorrection(cw, rng):
    """-> (received, other codeword): a column at distance 6 from the codeword cw and 5 from cw + w, w of weight 11 -- the
    decoder must return cw + w with a count of 5."""
    support = rng.choice(N, NPAR + 1, replace=False)
    w = min_weight_codeword(support, rng)
    r = cw.copy()
    r[support[:6]] ^= w[support[:6]]
    return r, cw ^ w


# error positions where decoders go wrong: the first and last byte, where data meets parity, all in the parity, adjacent
EDGE_ERROR_POSITIONS = [[], [0], [109], [110], [119], [0, 119], [109, 110], [0, 1, 2, 3, 4], [110, 113, 115, 117, 119],
                        [115, 116, 117, 118, 119], [107, 108, 109, 110, 111], [0, 59, 109, 110, 119], [3, 40, 77]]


# ----------------------------------------------------------------------------------------------- Fire code, AU CRC
FIRE_G = (1 << 16) | (1 << 14) | (1 << 13) | (1 << 12) | (1 << 11) | (1 << 5) | (1 << 3) | (1 << 2) | (1 << 1) | 1


def firecode(data):
    """Remainder of m(x) x^16 by G(x), m = the bytes MSB first (register started at zero)."""
    rem = 0
    for byte in bytes(bytearray(np.asarray(data, np.uint8))) + b"\0\0":   # two zero bytes: the message times x^16
        for bit in range(7, -1, -1):
            rem = (rem << 1) | ((byte >> bit) & 1)
            if rem & (1 << 16):
                rem ^= FIRE_G
    return rem


def au_crc(payload):
    return binascii.crc_hqx(bytes(bytearray(np.asarray(payload, np.uint8))), 0xFFFF) ^ 0xFFFF


# ------------------------------------------------------------------------------------------------------ super-frame
FIRST_START = {2: 5, 3: 6, 4: 8, 6: 11}           # header bytes: 2 Fire code + 1 + 12 bits per further AU start


def num_aus(dac_rate, sbr):
    """TS 102 563 table 2: 2 / 3 / 4 / 6 access units at 16 or 24 kHz AAC core, 32 or 48 kHz."""
    return {(0, 1): 2, (1, 1): 3, (0, 0): 4, (1, 0): 6}[(dac_rate, sbr)]


def superframe(sf, s):
    """One super-frame of 120 s bytes -> (corrected data part uint8[110 s], STATUS_DTYPE record).

    RS first, column by column (column j = bytes j, j + s, ...); a column that cannot be decoded is left as received.
    Then the header: the Fire code over bytes 2..10 must equal bytes 0..1, and an all-zero header is not a super-frame.
    Then the AU table: au_start[0] follows the header, au_start[1..n-1] are 12-bit fields from byte 3 on,
    au_start[n] = 110 s; an AU is checked only if start >= 3, end <= 110 s and end - start >= 3, and passes when the CRC
    of its payload equals its last two bytes."""
    sf = np.asarray(sf, np.uint8)
    assert sf.shape == (120 * s,)
    cols = sf.reshape(N, s).T.copy()                                  # [s][120]
    syn = syndromes(cols)
    st = np.zeros((), STATUS_DTYPE)
    for j in np.flatnonzero(syn.any(axis=1)):
        res = rs_decode(cols[j])
        if res is None:
            st["rs_uncorrectable"] += 1
        else:
            cols[j] = res[0]
            st["rs_corrected"] += res[1]
    data = cols.T.reshape(-1)[:110 * s].copy()
    fire_ok = bool(data[:11].any()) and firecode(data[2:11]) == (int(data[0]) << 8 | int(data[1]))
    st["firecode_ok"] = int(fire_ok)
    if not fire_ok:
        return data, st
    n = num_aus((int(data[2]) >> 6) & 1, (int(data[2]) >> 5) & 1)
    bits = np.unpackbits(data[3:11])
    starts = [FIRST_START[n]] + [int("".join(map(str, bits[12 * a:12 * a + 12])), 2) for a in range(n - 1)] + [110 * s]
    st["num_aus"] = n
    st["au_start"][:n + 1] = starts
    mask = 0
    for a in range(n):
        b0, b1 = starts[a], starts[a + 1]
        if b0 < 3 or b1 > 110 * s or b1 - b0 < 3:
            continue
        if au_crc(data[b0:b1 - 2]) == (int(data[b1 - 2]) << 8 | int(data[b1 - 1])):
            mask |= 1 << a
    st["au_crc_mask"] = mask
    return data, st


def superframes(sfs, s):
    """[n][>= 120 s] -> (data [n][110 s], status [n]) by superframe() on each row."""
    sfs = np.asarray(sfs, np.uint8)
    out = np.zeros((sfs.shape[0], 110 * s), np.uint8)
    st = np.zeros(sfs.shape[0], STATUS_DTYPE)
    for f in range(sfs.shape[0]):
        out[f], st[f] = superframe(sfs[f, :120 * s], s)
    return out, st
