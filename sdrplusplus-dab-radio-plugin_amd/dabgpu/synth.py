"""Synthetic DAB Mode-I transmitter (numpy) -- known-answer generator and bench input.

The reference ships no fixtures or tests; upstream DAB-Radio has a
`simulate_transmitter` example that is not in /root/reference.  This is an independent
restatement of the TRANSMIT side of ETSI EN 300 401 (clauses 5.2, 11, 12, 14), written
without sharing code or tables with oracle/ so that round trips cross-check both.

Frame layout produced: null symbol (2656 zeros) + PRS + 75 data symbols of 2552
samples = 196608 complex64 samples at 2.048 MSPS (what the plugin's VFO delivers,
/root/reference/src/dab_module.cpp:144-149).
"""
import numpy as np

NB_FFT = 2048
NB_CP = 504
NB_SYM = NB_FFT + NB_CP
NB_NULL = 2656
NB_SYMBOLS = 76
NB_CARRIERS = 1536
NB_SYM_BITS = 2 * NB_CARRIERS
NB_FRAME_BITS = 75 * NB_SYM_BITS
NB_FRAME_SAMPLES = NB_NULL + NB_SYMBOLS * NB_SYM
NB_FIC_BITS = 3 * NB_SYM_BITS
NB_CIF_BITS = 864 * 64
TDI_DELAY = np.array([0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15])

# generator polynomials, octal, MSB = current bit (clause 11.1.1)
_GEN_OCT = (0o133, 0o171, 0o145, 0o133)


# ----------------------------------------------------------------------------- tables
def carrier_of_data_index():
    """k_n (carrier number in [-768,768]\\{0}) for data index n (clause 14.6)."""
    pi = np.zeros(NB_FFT, np.int64)
    for i in range(1, NB_FFT):
        pi[i] = (13 * pi[i - 1] + 511) % NB_FFT
    keep = pi[(pi >= 256) & (pi <= 1792) & (pi != 1024)]
    return keep - 1024


def prs_carriers():
    """z_{1,k} for k=-768..768 (k=0 -> 0): dict-free dense array indexed k+768 (clause 14.3.2)."""
    h = np.array([
        [0, 2, 0, 0, 0, 0, 1, 1, 2, 0, 0, 0, 2, 2, 1, 1] * 2,
        [0, 3, 2, 3, 0, 1, 3, 0, 2, 1, 2, 3, 2, 3, 3, 0] * 2,
        [0, 0, 0, 2, 0, 2, 1, 3, 2, 2, 0, 2, 2, 0, 1, 3] * 2,
        [0, 1, 2, 1, 0, 3, 3, 2, 2, 3, 2, 1, 2, 1, 3, 2] * 2,
    ])
    # (k', i, n) Mode I, table 39
    rows = [(-768, 0, 1), (-736, 1, 2), (-704, 2, 0), (-672, 3, 1), (-640, 0, 3), (-608, 1, 2),
            (-576, 2, 2), (-544, 3, 3), (-512, 0, 2), (-480, 1, 1), (-448, 2, 2), (-416, 3, 3),
            (-384, 0, 1), (-352, 1, 2), (-320, 2, 3), (-288, 3, 3), (-256, 0, 2), (-224, 1, 2),
            (-192, 2, 2), (-160, 3, 1), (-128, 0, 1), (-96, 1, 3), (-64, 2, 1), (-32, 3, 2),
            (1, 0, 3), (33, 3, 1), (65, 2, 1), (97, 1, 1), (129, 0, 2), (161, 3, 2), (193, 2, 1),
            (225, 1, 0), (257, 0, 2), (289, 3, 2), (321, 2, 3), (353, 1, 3), (385, 0, 0),
            (417, 3, 2), (449, 2, 1), (481, 1, 3), (513, 0, 3), (545, 3, 3), (577, 2, 3),
            (609, 1, 0), (641, 0, 3), (673, 3, 0), (705, 2, 1), (737, 1, 1)]
    z = np.zeros(2 * 768 + 1, np.complex128)
    for kp, i, n in rows:
        for j in range(32):
            z[kp + j + 768] = 1j ** int((h[i][j] + n) % 4)
    return z


def puncture_vector(pi):
    order = [0, 4, 2, 6, 1, 5, 3, 7]
    ones = [1] * 8
    for s in range(pi):
        ones[order[s % 8]] += 1
    return np.array([[1 if b < ones[g] else 0 for b in range(4)] for g in range(8)], np.uint8).ravel()


def _mask_from_profile(blocks):
    parts = [np.tile(puncture_vector(pi), 4 * L) for L, pi in blocks if L > 0]
    parts.append(np.tile(np.array([1, 1, 0, 0], np.uint8), 6))
    return np.concatenate(parts)


def fic_mask():
    return _mask_from_profile([(21, 16), (3, 15)])


def eep_profile(option, level, bitrate):
    """-> (blocks [(L,PI),...], size_cu).  Clause 11.3.2."""
    if option == 0:
        n = bitrate // 8
        assert bitrate == 8 * n
        if level == 1:
            return [(6 * n - 3, 24), (3, 23)], 12 * n
        if level == 2:
            if n == 1:
                return [(5, 13), (1, 12)], 8
            return [(2 * n - 3, 14), (4 * n + 3, 13)], 8 * n
        if level == 3:
            return [(6 * n - 3, 8), (3, 7)], 6 * n
        if level == 4:
            return [(4 * n - 3, 3), (2 * n + 3, 2)], 4 * n
    else:
        n = bitrate // 32
        assert bitrate == 32 * n
        pis = {1: (10, 9), 2: (6, 5), 3: (4, 3), 4: (2, 1)}[level]
        cu = {1: 27, 2: 21, 3: 18, 4: 15}[level] * n
        return [(24 * n - 3, pis[0]), (3, pis[1])], cu
    raise ValueError("bad EEP profile")


def eep_mask(option, level, bitrate):
    blocks, cu = eep_profile(option, level, bitrate)
    m = _mask_from_profile(blocks)
    assert m.size == 4 * (bitrate * 24 + 6) and int(m.sum()) == cu * 64
    return m, cu


# UEP protection profiles (clause 11.3.1, Table 8) in table-index order: bitrate level size L1 L2 L3 L4 PI1 PI2 PI3 PI4
# padding.  Restated from memory; uep_profile() asserts the two identities every row must satisfy.
_UEP_TABLE = [tuple(int(v) for v in line.split()) for line in """
    32 5 16 3 4 17 0 5 3 2 0 0
    32 4 21 3 3 18 0 11 6 5 0 0
    32 3 24 3 4 14 3 15 9 6 8 0
    32 2 29 3 4 14 3 22 13 8 13 0
    32 1 35 3 5 13 3 24 17 12 17 4
    48 5 24 4 3 26 3 5 4 2 3 0
    48 4 29 3 4 26 3 9 6 4 6 0
    48 3 35 3 4 26 3 15 10 6 9 4
    48 2 42 3 4 26 3 24 14 8 15 0
    48 1 52 3 5 25 3 24 18 13 18 0
    56 5 29 6 10 23 3 5 4 2 3 0
    56 4 35 6 10 23 3 9 6 4 5 0
    56 3 42 6 12 21 3 16 7 6 9 0
    56 2 52 6 10 23 3 23 13 8 13 8
    64 5 32 6 9 31 2 5 3 2 3 0
    64 4 42 6 9 33 0 11 6 5 0 0
    64 3 48 6 12 27 3 16 8 6 9 0
    64 2 58 6 10 29 3 23 13 8 13 8
    64 1 70 6 11 28 3 24 18 12 18 4
    80 5 40 6 10 41 3 6 3 2 3 0
    80 4 52 6 10 41 3 11 6 5 6 0
    80 3 58 6 11 40 3 16 8 6 7 0
    80 2 70 6 10 41 3 23 13 8 13 8
    80 1 84 6 10 41 3 24 17 12 18 4
    96 5 48 7 9 53 3 5 4 2 4 0
    96 4 58 7 10 52 3 9 6 4 6 0
    96 3 70 6 12 51 3 16 9 6 10 4
    96 2 84 6 10 53 3 22 12 9 12 0
    96 1 104 6 13 50 3 24 18 13 19 0
    112 5 58 14 17 50 3 5 4 2 5 0
    112 4 70 11 21 49 3 9 6 4 8 0
    112 3 84 11 23 47 3 16 8 6 9 0
    112 2 104 11 21 49 3 23 12 9 14 4
    128 5 64 12 19 62 3 5 3 2 4 0
    128 4 84 11 21 61 3 11 6 5 7 0
    128 3 96 11 22 60 3 16 9 6 10 4
    128 2 116 11 21 61 3 22 12 9 14 0
    128 1 140 11 20 62 3 24 17 13 19 8
    160 5 80 11 19 87 3 5 4 2 4 0
    160 4 104 11 23 83 3 11 6 5 9 0
    160 3 116 11 24 82 3 16 8 6 11 0
    160 2 140 11 21 85 3 22 11 9 13 0
    160 1 168 11 22 84 3 24 18 12 19 0
    192 5 96 11 20 110 3 6 4 2 5 0
    192 4 116 11 22 108 3 10 6 4 9 0
    192 3 140 11 24 106 3 16 10 6 11 0
    192 2 168 11 20 110 3 22 13 9 13 8
    192 1 208 11 21 109 3 24 20 13 24 0
    224 5 116 12 22 131 3 8 6 2 6 4
    224 4 140 12 26 127 3 12 8 4 11 0
    224 3 168 11 20 134 3 16 10 7 9 0
    224 2 208 11 22 132 3 24 16 10 15 0
    224 1 232 11 24 130 3 24 20 12 20 4
    256 5 128 11 24 154 3 6 5 2 5 0
    256 4 168 11 24 154 3 12 9 5 10 4
    256 3 192 11 27 151 3 16 10 7 10 0
    256 2 232 11 22 156 3 24 14 10 13 8
    256 1 280 11 26 152 3 24 19 14 18 4
    320 5 160 11 26 200 3 8 5 2 6 4
    320 4 208 11 25 201 3 13 9 5 10 8
    320 2 280 11 26 200 3 24 17 9 17 0
    384 5 192 11 27 247 3 8 6 2 7 0
    384 3 280 11 24 250 3 16 9 7 10 4
    384 1 416 12 28 245 3 24 20 14 23 8
""".strip().splitlines()]


def uep_index(bitrate, level):
    for i, r in enumerate(_UEP_TABLE):
        if r[0] == bitrate and r[1] == level:
            return i
    raise ValueError("no UEP profile for %d kbit/s level %d" % (bitrate, level))


def uep_profile(index):
    """-> (blocks [(L,PI) x4], size_cu, padding_bits, bitrate)."""
    br, level, size, L1, L2, L3, L4, P1, P2, P3, P4, pad = _UEP_TABLE[index]
    blocks = [(L1, P1), (L2, P2), (L3, P3), (L4, P4)]
    assert sum(L for L, _ in blocks) * 32 == br * 24
    assert sum(L * (32 + 4 * P) for L, P in blocks) + 12 + pad == size * 64
    return blocks, size, pad, br


def uep_mask(index):
    blocks, cu, pad, br = uep_profile(index)
    m = _mask_from_profile(blocks)
    assert m.size == 4 * (br * 24 + 6) and int(m.sum()) + pad == cu * 64
    return m, cu


# ----------------------------------------------------------------------------- bit level
def prbs(n):
    reg = [1] * 9  # reg[0] newest
    out = np.zeros(n, np.uint8)
    for i in range(n):
        b = reg[8] ^ reg[4]
        out[i] = b
        reg = [b] + reg[:8]
    return out


def crc16(data):
    crc = 0xFFFF
    for byte in bytes(data):
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) if (crc & 0x8000) else (crc << 1)
            crc &= 0xFFFF
    return crc ^ 0xFFFF


def make_fibs(rng, n):
    """n random FIBs: 30 data bytes + CRC16 (clause 5.2.1)."""
    fibs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    for f in fibs:
        c = crc16(f[:30])
        f[30] = c >> 8
        f[31] = c & 0xFF
    return fibs


def conv_encode(bits):
    """rate-1/4 mother code with 6 zero tail bits -> 4*(n+6) bits, order x0,x1,x2,x3 per input."""
    a = np.concatenate([np.zeros(6, np.uint8), np.asarray(bits, np.uint8), np.zeros(6, np.uint8)])
    n = a.size - 6
    out = np.zeros((n, 4), np.uint8)
    for p, g in enumerate(_GEN_OCT):
        acc = np.zeros(n, np.uint8)
        for k in range(7):          # octal MSB (bit 6) multiplies a[i], bit (6-k) multiplies a[i-k]
            if (g >> (6 - k)) & 1:
                acc ^= a[6 - k: 6 - k + n]
        out[:, p] = acc
    return out.ravel()


def fic_encode(fibs12):
    """12 FIBs -> 9216 punctured coded bits (4 groups of 3 FIBs)."""
    m = fic_mask().astype(bool)
    pr = prbs(768)
    out = []
    for g in range(4):
        bits = np.unpackbits(np.asarray(fibs12[3 * g:3 * g + 3], np.uint8).ravel())
        out.append(conv_encode(bits ^ pr)[m])
    return np.concatenate(out)


def msc_encode_lf(lf_bytes, mask):
    """one logical frame of a subchannel -> punctured coded bits."""
    bits = np.unpackbits(np.asarray(lf_bytes, np.uint8))
    return conv_encode(bits ^ prbs(bits.size))[mask.astype(bool)]


def time_interleave(coded, cyclic=True):
    """coded [R][nbits] logical frames -> tx [R][nbits] CIF contents:
    tx[(r + d(i%16)) % R][i] = coded[r][i] (cyclic) ; non-cyclic leaves the first CIFs partly zero."""
    R, nbits = coded.shape
    tx = np.zeros_like(coded)
    d = TDI_DELAY[np.arange(nbits) % 16]
    for r in range(R):
        dst = r + d
        if cyclic:
            tx[dst % R, np.arange(nbits)] = coded[r]
        else:
            ok = dst < R
            tx[dst[ok], np.arange(nbits)[ok]] = coded[r][ok]
    return tx


# ----------------------------------------------------------------------------- OFDM
_CAR = None
_PRS = None


def _tables():
    global _CAR, _PRS
    if _CAR is None:
        _CAR = carrier_of_data_index()
        _PRS = prs_carriers()
    return _CAR, _PRS


#: transmitter identification (EN 300 401 section 14.8): the carrier bases of the four pair groups
TII_BASES = (-768, -384, 1, 385)


def tii_null(tii):
    """The null symbol [2656] complex64 of the transmitters `tii` = [(c, p) or (c, p, gain), ...]: comb c (sub-identifier),
    pattern p (main identifier, the p-th 8-bit value with four bits set, bit 7 - b = position b), complex amplitude gain
    (default 1).  Each switched-on pair k = B + 2c + 48b, k + 1 carries a data carrier's amplitude with the PRS phase of
    its carrier; the 2048-sample symbol is extended cyclically over the whole null period (a 608-sample prefix)."""
    _, prs = _tables()
    patterns = [v for v in range(256) if bin(v).count("1") == 4]
    spec = np.zeros(NB_FFT, np.complex128)
    for t in tii:
        c, p = int(t[0]), int(t[1])
        g = t[2] if len(t) > 2 else 1.0
        for b in range(8):
            if patterns[p] >> (7 - b) & 1:
                for base in TII_BASES:
                    for k in (base + 2 * c + 48 * b, base + 2 * c + 48 * b + 1):
                        spec[k % NB_FFT] += g * prs[k + 768]
    t = np.fft.ifft(spec) * (NB_FFT / np.sqrt(NB_CARRIERS))
    return t[(np.arange(NB_NULL) - (NB_NULL - NB_FFT)) % NB_FFT].astype(np.complex64)


def sfn(frame_bits, transmitters):
    """A single-frequency network: every transmitter sends the same frames (frame_bits [n][230400]) with its own TII.
    transmitters = [(c, p, delay in samples, gain in dB), ...] -> the sum as received, complex64 [n * 196608]
    (a delayed transmitter's first samples are zeros)."""
    frame_bits = np.asarray(frame_bits, np.uint8).reshape(-1, NB_FRAME_BITS)
    base = np.concatenate([modulate_frame(b) for b in frame_bits]).astype(np.complex128)
    out = np.zeros_like(base)
    for c, p, delay, gain_db in transmitters:
        x = base.copy()
        for f in range(frame_bits.shape[0]):
            x[f * NB_FRAME_SAMPLES:f * NB_FRAME_SAMPLES + NB_NULL] = tii_null([(c, p)])
        d = int(delay)
        out[d:] += 10.0 ** (gain_db / 20.0) * x[:x.size - d]
    return out.astype(np.complex64)


def modulate_frame(bits, tii=None):
    """230400 bits -> complex64[196608] (null + PRS + 75 symbols), unit average symbol power.  tii: the transmitters whose
    identification the null symbol carries (tii_null); None = a null symbol of zeros."""
    car, prs = _tables()
    bits = np.asarray(bits, np.uint8).reshape(75, NB_SYM_BITS)
    out = np.zeros(NB_FRAME_SAMPLES, np.complex64)
    if tii is not None:
        out[:NB_NULL] = tii_null(tii)
    z = prs.copy()                       # indexed k+768
    pos = NB_NULL
    scale = NB_FFT / np.sqrt(NB_CARRIERS)
    for l in range(NB_SYMBOLS):
        if l > 0:
            p = bits[l - 1].astype(np.float64)
            q = ((1 - 2 * p[:NB_CARRIERS]) + 1j * (1 - 2 * p[NB_CARRIERS:])) / np.sqrt(2.0)
            y = np.ones(2 * 768 + 1, np.complex128)
            y[car + 768] = q
            z = z * y
        spec = np.zeros(NB_FFT, np.complex128)
        k = np.arange(-768, 769)
        spec[k % NB_FFT] = z
        spec[0] = 0
        t = np.fft.ifft(spec) * scale
        out[pos:pos + NB_CP] = t[-NB_CP:]
        out[pos + NB_CP:pos + NB_SYM] = t
        pos += NB_SYM
    return out


_RESAMPLE_TAPS, _RESAMPLE_PHASES = 24, 2048


def _resample_table():
    """[phases + 1][taps] windowed-sinc (Kaiser, beta 8) interpolation weights: row q interpolates at a fraction q / phases
    between sample `half - 1` and `half` of its taps.  The DAB signal occupies 75 % of the band; with 24 taps and the
    fraction quantised to 1/2048 sample the interpolation error stays below -60 dB."""
    taps, ph = _RESAMPLE_TAPS, _RESAMPLE_PHASES
    half = taps // 2
    k = np.arange(-half + 1, half + 1, dtype=np.float64)
    frac = np.arange(ph + 1, dtype=np.float64)[:, None] / ph
    arg = k[None, :] - frac
    w = np.sinc(arg) * np.i0(8.0 * np.sqrt(np.clip(1.0 - (arg / (half + 0.5)) ** 2, 0.0, 1.0))) / np.i0(8.0)
    return (w / w.sum(axis=1, keepdims=True)).astype(np.float32)


def resample(x, ppm, chunk=1 << 20):
    """The stream as a receiver whose sample clock runs `ppm` parts per million FAST sees it: y[n] = x((n + 12) / (1 +
    ppm e-6)) -- more samples per transmitted frame, the frame period grows to 196608 (1 + ppm e-6) samples.
    x: complex numpy array, or a torch tensor (complex64, any device: long streams are resampled on the GPU)."""
    taps, ph = _RESAMPLE_TAPS, _RESAMPLE_PHASES
    half = taps // 2
    ratio = 1.0 / (1.0 + ppm * 1e-6)
    n_out = int(np.floor((x.shape[0] - 1) / ratio)) - taps
    table = _resample_table()
    if not isinstance(x, np.ndarray):                                # torch
        import torch
        tab = torch.from_numpy(table).to(x.device)
        k = torch.arange(-half + 1, half + 1, device=x.device)
        out = torch.empty(n_out, dtype=torch.complex64, device=x.device)
        for a in range(0, n_out, chunk):
            b = min(n_out, a + chunk)
            t = (torch.arange(a, b, dtype=torch.float64, device=x.device) + half) * ratio
            i0 = torch.floor(t).to(torch.int64)
            q = torch.round((t - i0) * ph).to(torch.int64)
            out[a:b] = (x[i0[:, None] + k[None, :]] * tab[q]).sum(dim=1)
        return out
    x = np.asarray(x, np.complex64)
    k = np.arange(-half + 1, half + 1)
    out = np.empty(n_out, np.complex64)
    for a in range(0, n_out, chunk):
        b = min(n_out, a + chunk)
        t = (np.arange(a, b, dtype=np.float64) + half) * ratio       # positions in x (shifted so that no index is < 0)
        i0 = np.floor(t).astype(np.int64)
        q = np.rint((t - i0) * ph).astype(np.int64)
        out[a:b] = (x[i0[:, None] + k[None, :]] * table[q]).sum(axis=1)
    return out


def fading_gain(n, rng, doppler, rice_k=4.0, fs=2.048e6, oscillators=8):
    """Slow flat fading: a line-of-sight component plus a sum of `oscillators` sinusoids with Doppler shifts up to
    `doppler` Hz (Jakes), unit mean power; rice_k = LOS / scattered power."""
    t = np.arange(n, dtype=np.float64) / fs
    g = np.zeros(n, np.complex128)
    for _ in range(oscillators):
        fd = doppler * np.cos(rng.uniform(0, 2 * np.pi))
        g += np.exp(1j * (2 * np.pi * fd * t + rng.uniform(0, 2 * np.pi)))
    g *= np.sqrt(1.0 / (oscillators * (rice_k + 1.0)))
    return g + np.sqrt(rice_k / (rice_k + 1.0))


def channel(iq, snr_db=None, cfo=0.0, rng=None, phase0=0.0, paths=None, sco_ppm=0.0, fading_hz=0.0, rice_k=4.0, gain=None):
    """The synthetic channel.  In the order a signal meets them:
      paths      multipath: [(delay in samples, complex gain), ...]; the first path is usually (0, 1).  The total is
                 normalised to unit power, so snr_db keeps its meaning.  None = one path.
      fading_hz  slow flat fading with this maximum Doppler shift (0 = none), Rice factor rice_k
      gain       optional per-sample real gain (array, e.g. a level step between frames)
      sco_ppm    sample-clock offset of the receiver (resample(): the frame period becomes 196608 (1 + ppm e-6) samples)
      cfo        carrier offset in cycles/sample, phase0 in cycles
      snr_db     AWGN relative to unit signal power (None = noiseless)"""
    x = np.asarray(iq, np.complex64).astype(np.complex128)
    if paths:
        y = np.zeros_like(x)
        norm = np.sqrt(sum(abs(g) ** 2 for _, g in paths))
        for d, g in paths:
            d = int(d)
            y[d:] += (g / norm) * x[:x.size - d]
        x = y
    if fading_hz > 0.0:
        x = x * fading_gain(x.size, rng, fading_hz, rice_k)
    if gain is not None:
        x = x * np.asarray(gain, np.float64)
    if sco_ppm != 0.0:
        x = resample(x, sco_ppm).astype(np.complex128)
    n = np.arange(x.size)
    if cfo != 0.0 or phase0 != 0.0:
        x = x * np.exp(2j * np.pi * (cfo * n + phase0))
    if snr_db is not None:
        sigma = np.sqrt(0.5 * 10 ** (-snr_db / 10))
        x = x + sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64)


class Ensemble:
    """A small cyclic multiplex: FIC of random FIBs + one EEP subchannel + random filler.

    `n_frames` frames form a cyclically time-interleaved stream (4*n_frames CIFs) so that
    tiling the frames back to back is a valid continuous transmission."""

    def __init__(self, seed, n_frames=4, option=0, level=3, bitrate=64, start_cu=0, uep_index=None):
        rng = np.random.default_rng(seed)
        self.n_frames = n_frames
        if uep_index is None:
            self.mask, self.size_cu = eep_mask(option, level, bitrate)
        else:                                    # UEP: the table row fixes bit rate, level and size
            self.mask, self.size_cu = uep_mask(uep_index)
            bitrate = _UEP_TABLE[uep_index][0]
        self.start_cu = start_cu
        self.lf_bytes = bitrate * 3
        R = 4 * n_frames
        self.fibs = make_fibs(rng, 12 * n_frames).reshape(n_frames, 12, 32)
        self.msc_bytes = rng.integers(0, 256, size=(R, self.lf_bytes), dtype=np.uint8)
        coded = np.stack([msc_encode_lf(self.msc_bytes[r], self.mask) for r in range(R)])
        if coded.shape[1] < self.size_cu * 64:   # UEP padding bits (zeros) fill the sub-channel
            coded = np.concatenate([coded, np.zeros((R, self.size_cu * 64 - coded.shape[1]), np.uint8)], axis=1)
        tx = time_interleave(coded, cyclic=True)
        cifs = rng.integers(0, 2, size=(R, NB_CIF_BITS), dtype=np.uint8)
        a = start_cu * 64
        cifs[:, a:a + self.size_cu * 64] = tx
        self.frame_bits = np.zeros((n_frames, NB_FRAME_BITS), np.uint8)
        for f in range(n_frames):
            self.frame_bits[f, :NB_FIC_BITS] = fic_encode(self.fibs[f])
            self.frame_bits[f, NB_FIC_BITS:] = cifs[4 * f:4 * f + 4].ravel()

    def iq(self):
        """[n_frames][196608] complex64."""
        return np.stack([modulate_frame(self.frame_bits[f]) for f in range(self.n_frames)])


class MultiEnsemble:
    """Cyclic multiplex with several EEP subchannels: specs = [(option, level, bitrate, start_cu), ...]."""

    def __init__(self, seed, specs, n_frames=4):
        rng = np.random.default_rng(seed)
        self.n_frames = n_frames
        self.specs = specs
        R = 4 * n_frames
        self.fibs = make_fibs(rng, 12 * n_frames).reshape(n_frames, 12, 32)
        cifs = rng.integers(0, 2, size=(R, NB_CIF_BITS), dtype=np.uint8)
        self.masks, self.sizes, self.msc_bytes = [], [], []
        for (option, level, bitrate, start_cu) in specs:
            mask, size_cu = eep_mask(option, level, bitrate)
            data = rng.integers(0, 256, size=(R, bitrate * 3), dtype=np.uint8)
            coded = np.stack([msc_encode_lf(data[r], mask) for r in range(R)])
            cifs[:, start_cu * 64:(start_cu + size_cu) * 64] = time_interleave(coded, cyclic=True)
            self.masks.append(mask); self.sizes.append(size_cu); self.msc_bytes.append(data)
        self.frame_bits = np.zeros((n_frames, NB_FRAME_BITS), np.uint8)
        for f in range(n_frames):
            self.frame_bits[f, :NB_FIC_BITS] = fic_encode(self.fibs[f])
            self.frame_bits[f, NB_FIC_BITS:] = cifs[4 * f:4 * f + 4].ravel()

    def iq(self):
        return np.stack([modulate_frame(self.frame_bits[f]) for f in range(self.n_frames)])


# ----------------------------------------------------------------------------- DAB+ audio super-frame (TS 102 563)
def _gf256():
    exp = np.zeros(512, np.int64)
    log = np.zeros(256, np.int64)
    x = 1
    for i in range(255):
        exp[i] = x
        log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    exp[255:510] = exp[:255]
    return exp, log


_GF_EXP, _GF_LOG = _gf256()


def _gf_mul(a, b):
    return 0 if a == 0 or b == 0 else int(_GF_EXP[_GF_LOG[a] + _GF_LOG[b]])


def _rs_generator():
    g = [1]                                   # g[i] = coefficient of x^i
    for k in range(10):
        nx = [0] * (len(g) + 1)
        for i, c in enumerate(g):
            nx[i + 1] ^= c
            nx[i] ^= _gf_mul(c, int(_GF_EXP[k]))
        g = nx
    return g


_RS_G = _rs_generator()


def rs_parity(data110):
    """RS(120,110) parity: remainder of d(x) x^10 by prod_{k=0..9}(x - alpha^k), GF(2^8) / 0x11D."""
    rem = [0] * 10                            # rem[0] = highest degree
    for d in data110:
        fb = int(d) ^ rem[0]
        rem = [rem[j + 1] ^ _gf_mul(fb, _RS_G[9 - j]) for j in range(9)] + [_gf_mul(fb, _RS_G[0])]
    return np.array(rem, np.uint8)


def firecode16(data):
    crc = 0
    for byte in bytes(data):
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x782F) if (crc & 0x8000) else (crc << 1)
            crc &= 0xFFFF
    return crc


def build_superframe(rng, bitrate, dac_rate=1, sbr=0, channel_mode=1, ps=0, cuts=None, bodies=None):
    """-> (sf uint8[120*s], au_start list with the end appended, list of AU payloads incl. CRC).
    cuts: the start addresses of access units 1 .. n-1 (default: drawn at random).
    bodies: per access unit, the bytes its body begins with (au_body: a data stream element carrying PAD) or None; the
    random body is drawn as without, then its beginning is overwritten, so the draws do not depend on `bodies`."""
    s = bitrate // 8
    size = 110 * s
    num_aus = {(0, 1): 2, (1, 1): 3, (0, 0): 4, (1, 0): 6}[(dac_rate, sbr)]
    first = {2: 5, 3: 6, 4: 8, 6: 11}[num_aus]
    if cuts is None:                          # (the header holds 12-bit starts: below 4096 from s = 38 on)
        cuts = np.sort(rng.choice(np.arange(first + 8, min(size - 8, 4096), 4), num_aus - 1, replace=False))
    assert len(cuts) == num_aus - 1 and all(first + 3 <= c < 4096 for c in cuts) and all(b - a >= 3 for a, b in zip(cuts, list(cuts[1:]) + [size]))
    starts = [first] + [int(c) for c in cuts] + [size]
    sf = np.zeros(120 * s, np.uint8)
    sf[2] = (dac_rate << 6) | (sbr << 5) | (channel_mode << 4) | (ps << 3)
    bits = []
    for a in range(1, num_aus):
        bits += [(starts[a] >> (11 - b)) & 1 for b in range(12)]
    bits += [0] * ((-len(bits)) % 8)
    hdr = np.packbits(np.array(bits, np.uint8)) if bits else np.zeros(0, np.uint8)
    sf[3:3 + hdr.size] = hdr
    aus = []
    for a in range(num_aus):
        body = rng.integers(0, 256, starts[a + 1] - starts[a] - 2, dtype=np.uint8)
        if bodies is not None and bodies[a] is not None:
            head = np.frombuffer(bytes(bodies[a]), np.uint8)
            assert head.size <= body.size, "access unit %d has %d bytes, its PAD element %d" % (a, body.size, head.size)
            body[:head.size] = head
        c = crc16(body)
        au = np.concatenate([body, np.array([c >> 8, c & 0xFF], np.uint8)])
        sf[starts[a]:starts[a + 1]] = au
        aus.append(au)
    fc = firecode16(sf[2:11])
    sf[0], sf[1] = fc >> 8, fc & 0xFF
    for j in range(s):
        sf[size + j::s] = rs_parity(sf[j:size:s])
    return sf, starts, aus


# ----------------------------------------------------------------------------- PAD: dynamic label (EN 300 401 7.4, TS 102 563 5.4)
# The transmit side of the dynamic label, from the clauses: label -> segments (data groups with toggle, first / last flags
# and CRC) -> X-PAD sub-fields, short or variable -> PAD (X-PAD bytes in reverse order, then F-PAD) -> data stream element
# -> the beginning of an access unit's body (build_superframe's `bodies`).
XPAD_LENGTHS = (4, 6, 8, 12, 16, 24, 32, 48)
XPAD_DLS_START, XPAD_DLS_CONT = 2, 3
CHARSET_EBU_LATIN, CHARSET_UCS2, CHARSET_UTF8 = 0, 6, 15


def dls_group(b0, b1, body=b""):
    """one DLS data group: the two prefix bytes, the body, the CRC (the FIB's, big-endian)"""
    g = bytes([b0 & 0xFF, b1 & 0xFF]) + bytes(body)
    c = crc16(g)
    return g + bytes([c >> 8, c & 0xFF])


def dls_segment(data, number, toggle, first, last, charset=CHARSET_UTF8):
    """segment `number` of a label: 1 .. 16 bytes; the first one carries the charset where the others carry their number"""
    data = bytes(data)
    assert 1 <= len(data) <= 16 and 0 <= number <= 7
    b0 = (toggle << 7) | (int(first) << 6) | (int(last) << 5) | (len(data) - 1)
    return dls_group(b0, ((charset if first else number) & 0x0F) << 4, data)


def dls_segments(text, toggle=0, charset=CHARSET_UTF8, seg_bytes=16):
    """the label's bytes (at most 128; at most 8 segments) cut into segments of seg_bytes -> list of data groups"""
    text = bytes(text)
    assert 1 <= len(text) <= 128 and 1 <= seg_bytes <= 16
    parts = [text[i:i + seg_bytes] for i in range(0, len(text), seg_bytes)]
    assert len(parts) <= 8
    return [dls_segment(part, m, toggle, m == 0, m == len(parts) - 1, charset) for m, part in enumerate(parts)]


def dls_command(command, toggle=0, body=b""):
    """a command group: 1 = clear (no body), 2 = DL Plus (1 .. 16 bytes of body), anything else for a receiver to ignore"""
    b0 = (toggle << 7) | 0x10 | (command & 0x0F)
    if command == 2:
        assert 1 <= len(body) <= 16
        return dls_group(b0, (len(body) - 1) & 0x0F, body)
    return dls_group(b0, 0, body)


def xpad_variable(subfields, end_marker=True):
    """variable-size X-PAD with content indicators: subfields = [(type, data)] or [(31, extended type, data)], at most four,
    every data a length of XPAD_LENGTHS -> the logical bytes: the list (closed by the end marker when shorter than four and
    asked for), then the data"""
    assert 1 <= len(subfields) <= 4
    out, tail = [], b""
    for sf in subfields:
        typ, data = sf[0], bytes(sf[-1])
        out.append((XPAD_LENGTHS.index(len(data)) << 5) | (typ & 0x1F))
        if typ == 31:
            out.append(sf[1] & 0xFF)
        tail += data
    if len(subfields) < 4 and end_marker:
        out.append(0)
    return bytes(out) + tail


def xpad_short(data, app_type=None):
    """short X-PAD: with a content indicator (app_type) 3 data bytes, without 4"""
    data = bytes(data)
    if app_type is None:
        assert len(data) == 4
        return data
    assert len(data) == 3
    return bytes([app_type & 0x1F]) + data


def pad_field(xpad, ind, ci, n=None, fpad_type=0):
    """PAD of n bytes (default: no more than needed): the X-PAD logical bytes in reverse order in front of the two F-PAD
    bytes; what n leaves over lies in front of them (logical bytes behind the field's own)"""
    xpad = bytes(xpad)
    n = len(xpad) + 2 if n is None else n
    assert n >= len(xpad) + 2
    fpad = bytes([(fpad_type << 6) | (ind << 4), (int(ci) << 1)])
    return bytes(n - 2 - len(xpad)) + xpad[::-1] + fpad


def dse(pad, tag=0, escape=None):
    """the data stream element that carries PAD: id 4, instance tag, no alignment flag, count (with the escape byte from
    255 bytes on), the bytes"""
    pad = bytes(pad)
    assert len(pad) <= 510
    if escape is None:
        escape = len(pad) >= 255
    assert escape == (len(pad) >= 255), "the escape byte is there exactly from 255 bytes on"
    head = bytes([(4 << 5) | ((tag & 0x0F) << 1)])
    return head + (bytes([255, len(pad) - 255]) if escape else bytes([len(pad)])) + pad


def dls_subfields(group, lengths, first_type=XPAD_DLS_START):
    """a data group cut into sub-fields of the given lengths (the last one filled up with zeros): [(type, data)] -- the
    first of type 2, the others of type 3; as many as the group needs"""
    group, out, at, k = bytes(group), [], 0, 0
    while at < len(group):
        n = lengths[min(k, len(lengths) - 1)]
        part = group[at:at + n]
        out.append((first_type if k == 0 else XPAD_DLS_CONT, part + bytes(n - len(part))))
        at += n
        k += 1
    return out


def dls_pads(groups, length_index=None, ci_less=False, before=(), after=(), end_marker=True, n=None):
    """One PAD field per access unit for a sequence of data groups, one DLS sub-field per access unit.
    length_index None: short X-PAD (the first access unit of a group has the content indicator and 3 bytes, the others are
    CI-less with 4).  Else variable X-PAD with sub-fields of XPAD_LENGTHS[length_index]; ci_less: the continuation
    sub-fields go without a list; before / after: other applications' sub-fields [(type, data)] around the DLS one in
    every list (a CI-less field continues the LAST sub-field of the list, so `after` and ci_less exclude each other);
    either may be a callable, PAD index -> sub-fields (those of mot_fields: one PAD for a label and a slide)."""
    assert not (ci_less and after)
    pads = []
    at_pad = lambda fields: list(fields(len(pads)) if callable(fields) else fields)    # (a callable: PAD index -> sub-fields)
    for g in groups:
        if length_index is None:
            g = bytes(g)
            pads.append(pad_field(xpad_short(g[:3] + bytes(3 - len(g[:3])), XPAD_DLS_START), 1, 1, n))
            for at in range(3, len(g), 4):
                part = g[at:at + 4]
                pads.append(pad_field(xpad_short(part + bytes(4 - len(part))), 1, 0, n))
            continue
        for k, (typ, data) in enumerate(dls_subfields(g, [XPAD_LENGTHS[length_index]])):
            if k and ci_less:
                pads.append(pad_field(data, 2, 0, n))
            else:
                pads.append(pad_field(xpad_variable(at_pad(before) + [(typ, data)] + at_pad(after), end_marker), 2, 1, n))
    return pads


def au_body(pad, tag=0):
    """what an access unit's body begins with to carry this PAD (build_superframe's `bodies`); None for no PAD"""
    return None if pad is None else dse(pad, tag)


# ----------------------------------------------------------------------------- DAB (MPEG layer II) audio frames
# The transmit side of include/dabgpu_mp2_frame.h, from the clauses: header (ISO 11172-3 2.4.1.3), CRC, bit allocation and
# SCFSI (2.4.1.4 - 2.4.1.6, Annex B table B.2), then a random body, the ScF-CRC bytes and the PAD at the frame's end
# (EN 300 401 7.3.1.5, 7.4.1).
MP2_RATES_48K = (0, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384)
MP2_RATES_24K = (0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160)
MP2_STEREO, MP2_JOINT, MP2_DUAL, MP2_MONO = 0, 1, 2, 3
_MP2_NBAL_48K_SMALL = [4] * 2 + [3] * 6
_MP2_NBAL_48K_LARGE = [4] * 11 + [3] * 12 + [2] * 4
_MP2_NBAL_24K = [4] * 4 + [3] * 7 + [2] * 19


def _mp2_crc_table():
    t = []
    for v in range(256):
        r = v << 8
        for _ in range(8):
            r = ((r << 1) ^ 0x8005) & 0xFFFF if r & 0x8000 else (r << 1) & 0xFFFF
        t.append(r)
    return t


_MP2_CRC_TABLE = _mp2_crc_table()


def mp2_crc(bits):
    """the ISO 11172-3 CRC-16 (0x8005, start 0xFFFF) over a list of bits: whole bytes through the table, the rest by shifts"""
    crc, n = 0xFFFF, len(bits) // 8 * 8
    for at in range(0, n, 8):
        v = int("".join(str(int(b)) for b in bits[at:at + 8]), 2)
        crc = ((crc << 8) & 0xFFFF) ^ _MP2_CRC_TABLE[(crc >> 8) ^ v]
    for b in bits[n:]:
        crc = ((crc << 1) & 0xFFFF) ^ (0x8005 if ((crc >> 15) ^ int(b)) & 1 else 0)
    return crc


def mp2_scf_crc_bytes(bitrate, mode, lsf):
    per_channel = bitrate if mode == MP2_MONO else bitrate // 2
    return 4 if lsf or per_channel >= 56 else 2


def mp2_frame(rng, bitrate, mode=MP2_STEREO, mode_ext=0, lsf=False, pad=None, crc=True, silent_bands=0.25):
    """One layer-II audio frame as a DAB sub-channel of `bitrate` kbit/s carries it: 3 * bitrate bytes at 48 kHz, 6 * bitrate
    (two logical frames) at 24 kHz (lsf) -- header, a correct ISO CRC (crc=False: protection bit 1, no CRC), random bit
    allocation (a share of silent_bands of the fields zero), random SCFSI and body, and `pad` -- pad_field()'s bytes: the
    X-PAD in reverse order, then the two F-PAD bytes -- at the frame's end: F-PAD last, four X-PAD bytes in front of it,
    the rest in front of the ScF-CRC bytes.  None: the random body stands there."""
    rates = MP2_RATES_24K if lsf else MP2_RATES_48K
    assert bitrate in rates[1:], "no bit-rate index names %d kbit/s" % bitrate
    if not lsf:                                                     # ISO 11172-3 2.4.2.3
        assert not (bitrate in (32, 48, 56, 80) and mode != MP2_MONO) and not (bitrate in (224, 256, 320, 384) and mode == MP2_MONO)
    L = (6 if lsf else 3) * bitrate
    f = rng.integers(0, 256, size=L, dtype=np.uint8)
    f[0] = 0xFF
    f[1] = 0xF0 | ((0 if lsf else 1) << 3) | (2 << 1) | (0 if crc else 1)
    f[2] = (rates.index(bitrate) << 4) | (1 << 2) | (int(f[2]) & 1)
    f[3] = (mode << 6) | (mode_ext << 4) | (int(f[3]) & 0x0F)
    channels = 1 if mode == MP2_MONO else 2
    per_channel = bitrate // channels
    nbal = _MP2_NBAL_24K if lsf else _MP2_NBAL_48K_SMALL if per_channel in (32, 48) else _MP2_NBAL_48K_LARGE
    bound = min(4 * (mode_ext + 1), len(nbal)) if mode == MP2_JOINT else len(nbal)
    bits, scfsi = [], 0
    for sb, n in enumerate(nbal):
        shared = channels == 2 and sb >= bound
        for _ in range(1 if channels == 1 or shared else 2):
            a = 0 if rng.random() < silent_bands else int(rng.integers(1, 1 << n))
            bits += [(a >> (n - 1 - k)) & 1 for k in range(n)]
            scfsi += (2 if shared else 1) * (a != 0)
    bits += [int(b) for b in rng.integers(0, 2, size=2 * scfsi)]
    if crc:
        nbytes = (len(bits) + 7) // 8
        stream = np.unpackbits(f[6:6 + nbytes])
        stream[:len(bits)] = bits
        f[6:6 + nbytes] = np.packbits(stream)
        head = [int(b) for b in np.unpackbits(f[2:4])]
        c = mp2_crc(head + bits)
        f[4], f[5] = c >> 8, c & 0xFF
    if pad is not None:
        pad = bytes(pad)
        c = mp2_scf_crc_bytes(bitrate, mode, lsf)
        xpad = pad[:-2]
        assert len(pad) >= 2 and len(xpad) <= min(196, L - 8 - c), "the PAD does not fit this frame"
        xpad = bytes(max(0, 4 - len(xpad))) + xpad
        f[L - 2:] = np.frombuffer(pad[-2:], np.uint8)
        f[L - 6:L - 2] = np.frombuffer(xpad[-4:], np.uint8)
        if len(xpad) > 4:
            f[L - 6 - c - (len(xpad) - 4):L - 6 - c] = np.frombuffer(xpad[:-4], np.uint8)
    return f


# The transmit side of include/dabgpu_mp2_audio.h: a frame whose whole audio part is chosen -- bit allocation, SCFSI, scale
# factors and samples (ISO 11172-3 2.4.1.6, Annex B tables B.2a, B.2c and B.4; ISO 13818-3 table B.1) -- and the sub-band
# values those choices mean.  Levels of allocation index 1, 2, ... per run of sub-bands:
_MP2_LEVELS_48K_LARGE = ([[3] + [2 ** b - 1 for b in range(3, 17)]] * 3
                         + [[3, 5, 7, 9] + [2 ** b - 1 for b in range(4, 14)] + [65535]] * 8
                         + [[3, 5, 7, 9, 15, 31, 65535]] * 12 + [[3, 5, 65535]] * 4)
_MP2_LEVELS_48K_SMALL = [[3, 5, 9] + [2 ** b - 1 for b in range(4, 16)]] * 2 + [[3, 5, 9, 15, 31, 63, 127]] * 6
_MP2_LEVELS_24K = [[3, 5, 7, 9] + [2 ** b - 1 for b in range(4, 15)]] * 4 + [[3, 5, 9, 15, 31, 63, 127]] * 7 + [[3, 5, 9]] * 19
_MP2_GROUPED_BITS = {3: 5, 5: 7, 9: 10}
_MP2_SCF_PARTS = {0: (0, 1, 2), 1: (0, 0, 1), 2: (0, 0, 0), 3: (0, 1, 1)}     # SCFSI -> which index sent holds in each part


def mp2_levels(bitrate, mode, lsf):
    """levels[sb][a - 1] of the allocation table a frame of this rate and mode uses"""
    per_channel = bitrate if mode == MP2_MONO else bitrate // 2
    return _MP2_LEVELS_24K if lsf else _MP2_LEVELS_48K_SMALL if per_channel in (32, 48) else _MP2_LEVELS_48K_LARGE


def mp2_field_bits(n):
    """bits an active allocation field of n levels takes in one granule"""
    return _MP2_GROUPED_BITS[n] if n in _MP2_GROUPED_BITS else 3 * (n + 1).bit_length() - 3


def mp2_audio_bits(bitrate, mode, mode_ext, lsf, alloc, scfsi):
    """(E, limit): the bit position behind the last sample of a frame with allocation indices alloc[ch][sb] and SCFSI
    scfsi[ch][sb], and the position its audio must end in front of, 8 (L - 6 - c)"""
    levels = mp2_levels(bitrate, mode, lsf)
    channels, sblimit = (1 if mode == MP2_MONO else 2), len(levels)
    bound = min(4 * (mode_ext + 1), sblimit) if mode == MP2_JOINT else sblimit
    nbal = [len(l).bit_length() for l in levels]
    E = 48
    for sb in range(sblimit):
        shared = channels == 2 and sb >= bound
        for ch in range(channels):
            a = int(alloc[0 if shared else ch][sb])
            if not shared or ch == 0:
                E += nbal[sb] + (12 * mp2_field_bits(levels[sb][a - 1]) if a else 0)
            if a:
                E += 2 + 6 * len(set(_MP2_SCF_PARTS[int(scfsi[ch][sb])]))
    return E, 8 * ((6 if lsf else 3) * bitrate - 6 - mp2_scf_crc_bytes(bitrate, mode, lsf))


def mp2_audio_pack(rng, bitrate, mode, mode_ext, lsf, alloc, scfsi, scf, samples, pad=None, codes=None, fit=True):
    """The frame that says exactly this: allocation indices alloc[ch][sb] (a shared field is channel 0's), SCFSI
    scfsi[ch][sb], scale-factor indices scf[ch][sb][part] (of which the frame sends those its SCFSI names: for SCFSI 1 the
    indices of parts 0 and 2, for 2 that of part 0, for 3 those of parts 0 and 1) and samples[ch][t][sb] (integers 0 .. n - 1;
    a shared field carries channel 0's) -- or, for a grouped field, codes[(g, sb, ch)] = the raw code word instead of its
    three samples.  Header, ISO CRC, the audio from bit 48 on, random bytes behind it (rng), the PAD as mp2_frame lays it.
    fit = False packs an audio part that runs past 8 (L - 6 - c), as far as the frame goes.
    -> (frame uint8 [L], truth float64 [2][36][32]: what the frame's words mean, read as the frame sends them)"""
    rates = MP2_RATES_24K if lsf else MP2_RATES_48K
    assert bitrate in rates[1:]
    L = (6 if lsf else 3) * bitrate
    levels = mp2_levels(bitrate, mode, lsf)
    channels, sblimit = (1 if mode == MP2_MONO else 2), len(levels)
    bound = min(4 * (mode_ext + 1), sblimit) if mode == MP2_JOINT else sblimit
    nbal = [len(l).bit_length() for l in levels]
    E, limit = mp2_audio_bits(bitrate, mode, mode_ext, lsf, alloc, scfsi)
    assert not fit or E <= limit, "the audio does not fit: %d bits in front of %d" % (E, limit)
    f = rng.integers(0, 256, size=L, dtype=np.uint8)
    f[0] = 0xFF
    f[1] = 0xF0 | ((0 if lsf else 1) << 3) | (2 << 1)
    f[2] = (rates.index(bitrate) << 4) | (1 << 2) | (int(f[2]) & 1)
    f[3] = (mode << 6) | (mode_ext << 4) | (int(f[3]) & 0x0F)
    bits = []

    def put(v, n):
        bits.extend((int(v) >> (n - 1 - k)) & 1 for k in range(n))

    fields = [(sb, ch) for sb in range(sblimit) for ch in range(1 if channels == 1 or sb >= bound else 2)]
    cells = [(sb, ch) for sb in range(sblimit) for ch in range(channels)]
    index = lambda sb, ch: int(alloc[0 if channels == 2 and sb >= bound else ch][sb])
    for sb, ch in fields:
        put(index(sb, ch), nbal[sb])
    active = [(sb, ch) for sb, ch in cells if index(sb, ch)]
    for sb, ch in active:
        put(scfsi[ch][sb], 2)
    protected = len(bits)
    for sb, ch in active:
        parts = _MP2_SCF_PARTS[int(scfsi[ch][sb])]
        for j in sorted(set(parts)):
            put(scf[ch][sb][parts.index(j)], 6)
    truth = np.zeros((2, 36, 32), np.float64)
    for g in range(12):
        for sb, ch in fields:
            a = index(sb, ch)
            if not a:
                continue
            n = levels[sb][a - 1]
            if n in _MP2_GROUPED_BITS:
                if codes is not None and (g, sb, ch) in codes:
                    c = int(codes[(g, sb, ch)])
                else:
                    c = sum(int(samples[ch][3 * g + k][sb]) * n ** k for k in range(3))
                put(c, _MP2_GROUPED_BITS[n])
                s = [c % n, (c // n) % n, (c // (n * n)) % n]
            else:
                s = [int(samples[ch][3 * g + k][sb]) for k in range(3)]
                for v in s:
                    put(v, (n + 1).bit_length() - 1)
            for to in ((0, 1) if channels == 2 and sb >= bound else (ch,)):
                # (the index that holds in this part is the one SENT for it: parts that share an index share the first's)
                parts = _MP2_SCF_PARTS[int(scfsi[to][sb])]
                i = int(scf[to][sb][parts.index(parts[g // 4])])
                factor = 0.0 if i == 63 else 2.0 ** (1.0 - i / 3.0)
                for k in range(3):
                    truth[to, 3 * g + k, sb] = (2 * s[k] + 1 - n) / n * factor
    assert len(bits) == E - 48
    bits = bits[:8 * (L - 6)]
    nbytes = (len(bits) + 7) // 8
    stream = np.unpackbits(f[6:6 + nbytes])
    stream[:len(bits)] = bits
    f[6:6 + nbytes] = np.packbits(stream)
    c = mp2_crc([int(b) for b in np.unpackbits(f[2:4])] + bits[:protected])
    f[4], f[5] = c >> 8, c & 0xFF
    if pad is not None:
        pad = bytes(pad)
        c = mp2_scf_crc_bytes(bitrate, mode, lsf)
        xpad = pad[:-2]
        assert len(pad) >= 2 and len(xpad) <= min(196, L - 8 - c), "the PAD does not fit this frame"
        xpad = bytes(max(0, 4 - len(xpad))) + xpad
        f[L - 2:] = np.frombuffer(pad[-2:], np.uint8)
        f[L - 6:L - 2] = np.frombuffer(xpad[-4:], np.uint8)
        if len(xpad) > 4:
            assert 8 * (L - 6 - c - (len(xpad) - 4)) >= min(E, limit), "the PAD would lie over the audio"
            f[L - 6 - c - (len(xpad) - 4):L - 6 - c] = np.frombuffer(xpad[:-4], np.uint8)
    return f, truth


def mp2_audio_frame(rng, bitrate, mode=MP2_STEREO, mode_ext=0, lsf=False, pad=None, silent_bands=0.25, scf_range=(0, 63)):
    """One layer-II audio frame with a whole audio part, and the truth: random allocation (a share of silent_bands of the
    fields zero), SCFSI, scale-factor indices (scf_range, 63 excluded) and samples; the largest allocation indices are lowered
    one at a time until the audio (and an X-PAD of more than four bytes) fits in front of L - 6 - c.
    -> (frame uint8 [L], truth float64 [2][36][32]) as mp2_audio_pack."""
    levels = mp2_levels(bitrate, mode, lsf)
    channels, sblimit = (1 if mode == MP2_MONO else 2), len(levels)
    bound = min(4 * (mode_ext + 1), sblimit) if mode == MP2_JOINT else sblimit
    alloc = np.zeros((2, 32), np.int64)
    for sb in range(sblimit):
        for ch in range(channels):
            if rng.random() >= silent_bands:
                alloc[ch][sb] = rng.integers(1, len(levels[sb]) + 1)
        if channels == 2 and sb >= bound:
            alloc[1][sb] = alloc[0][sb]
    scfsi = rng.integers(0, 4, size=(2, 32))
    scf = rng.integers(scf_range[0], scf_range[1], size=(2, 32, 3))
    room = 8 * max(0, len(bytes(pad)) - 2 - 4) if pad is not None else 0
    while True:
        E, limit = mp2_audio_bits(bitrate, mode, mode_ext, lsf, alloc, scfsi)
        if E <= limit - room:
            break
        ch, sb = np.unravel_index(int(np.argmax(alloc)), alloc.shape)      # (the first of the largest)
        alloc[ch][sb] -= 1
        if channels == 2 and sb >= bound:
            alloc[1][sb] = alloc[0][sb]
    samples = np.zeros((2, 36, 32), np.int64)
    for sb in range(sblimit):
        for ch in range(channels):
            if alloc[ch][sb]:
                samples[ch, :, sb] = rng.integers(0, levels[sb][alloc[ch][sb] - 1], size=36)
    return mp2_audio_pack(rng, bitrate, mode, mode_ext, lsf, alloc, scfsi, scf, samples, pad=pad)


# ----------------------------------------------------------------------------- PAD: slideshow (MOT in X-PAD)
# The transmit side of the slideshow, from the clauses: object -> MOT header (core + parameters, EN 301 234 6.1, 6.2;
# TS 101 499 6.2) and body -> segments with their segmentation header (EN 301 234 5.1) -> MSC data groups with session
# header and CRC (EN 300 401 5.3.3) -> X-PAD sub-fields: the data group length indicator (type 1), then the group in
# sub-fields of type 12 (start) and 13 (continuation) (EN 300 401 7.4.5.1).
XPAD_DGLI, XPAD_MOT_START, XPAD_MOT_CONT = 1, 12, 13
MOT_DG_HEADER, MOT_DG_BODY = 3, 4
MOT_CONTENT_NAME, MOT_TRIGGER_TIME, MOT_EXPIRE_TIME = 0x0C, 0x05, 0x04
MOT_CATEGORY_SLIDE_ID, MOT_CATEGORY_TITLE, MOT_CLICK_THROUGH_URL, MOT_ALTERNATIVE_LOCATION_URL = 0x25, 0x26, 0x27, 0x28


def mot_param(param_id, data=b"", pli=None, long_length=None):
    """one header extension parameter: PLI 0 / 1 / 2 for no / one / four data bytes, else PLI 3 with a length of 7 bits, or
    of 15 (long_length; default from 128 bytes on).  pli = 3 forces the length form on short data."""
    data = bytes(data)
    if pli is None:
        pli = {0: 0, 1: 1, 4: 2}.get(len(data), 3)
    assert {0: len(data) == 0, 1: len(data) == 1, 2: len(data) == 4, 3: len(data) < 32768}[pli]
    head = bytes([(pli << 6) | (param_id & 0x3F)])
    if pli < 3:
        return head + data
    if long_length is None:
        long_length = len(data) >= 128
    assert long_length or len(data) < 128
    return head + (bytes([0x80 | (len(data) >> 8), len(data) & 0xFF]) if long_length else bytes([len(data)])) + data


def mot_time(mjd_day=None, hours=0, minutes=0):
    """the four bytes of a short-form time: validity(1) MJD(17) rfu(2) UTC flag(1) = 0, hours(5) minutes(6); None = "now":
    validity clear and every other bit zero"""
    if mjd_day is None:
        return bytes(4)
    v = (1 << 31) | ((mjd_day & 0x1FFFF) << 14) | ((hours & 0x1F) << 6) | (minutes & 0x3F)
    return v.to_bytes(4, "big")


def mot_header(body_size, content_type, content_subtype, params=(), header_size=None):
    """header core (BodySize 28, HeaderSize 13, ContentType 6, ContentSubType 9 bits) and the header extension
    (params: encoded by mot_param); header_size: what the core says (default: the truth)"""
    ext = b"".join(bytes(p) for p in params)
    size = 7 + len(ext) if header_size is None else header_size
    assert body_size < 1 << 28 and size < 1 << 13
    core = (body_size << 28) | (size << 15) | ((content_type & 0x3F) << 9) | (content_subtype & 0x1FF)
    return core.to_bytes(7, "big") + ext


def slide_header(body_size, name, subtype=1, charset=CHARSET_UTF8, trigger="now", extra=()):
    """the MOT header of a slide: an image (content type 2; subtype 1 JFIF, 3 PNG) with its ContentName and TriggerTime"""
    params = [mot_param(MOT_CONTENT_NAME, bytes([charset << 4]) + bytes(name))]
    if trigger is not None:
        params.append(mot_param(MOT_TRIGGER_TIME, mot_time() if trigger == "now" else bytes(trigger)))
    return mot_header(body_size, 2, subtype, params + list(extra))


def mot_segments(data, seg_size):
    """an object part cut into segments of seg_size (the last one shorter or equal; one empty segment for no bytes)"""
    data = bytes(data)
    assert 1 <= seg_size <= 8191
    return [data[i:i + seg_size] for i in range(0, len(data), seg_size)] or [b""]


def msc_data_group(dg_type, data, tid=None, segment=None, continuity=0, repetition=0, extension=None, end_user=b"",
                   crc=True, user_access=None):
    """one MSC data group: header (extension flag, CRC flag, segment flag, user access flag, type; continuity and
    repetition index; the extension field), session header (segment = (number, last); user access field with transport
    id and end-user address), the data field, the CRC (the FIB's, big-endian).  user_access: default when tid is given;
    True with tid None sends the field with its transport id flag clear."""
    if user_access is None:
        user_access = tid is not None
    b0 = ((extension is not None) << 7) | (int(crc) << 6) | ((segment is not None) << 5) | (int(user_access) << 4) | (dg_type & 0x0F)
    g = bytes([b0, ((continuity & 0x0F) << 4) | (repetition & 0x0F)])
    if extension is not None:
        g += int(extension).to_bytes(2, "big")
    if segment is not None:
        number, last = segment
        g += ((int(last) << 15) | (number & 0x7FFF)).to_bytes(2, "big")
    if user_access:
        end_user = bytes(end_user)
        li = (2 if tid is not None else 0) + len(end_user)
        assert li <= 15
        g += bytes([((tid is not None) << 4) | li]) + (int(tid).to_bytes(2, "big") if tid is not None else b"") + end_user
    g += bytes(data)
    if crc:
        c = crc16(g)
        g += bytes([c >> 8, c & 0xFF])
    return g


def mot_group(dg_type, tid, number, last, segment, repetition_count=0, size=None, **kw):
    """a MOT segment in its data group: the segmentation header (RepetitionCount 3, SegmentSize 13 bits; size: what it
    says, default the truth) in front of the segment"""
    segment = bytes(segment)
    size = len(segment) if size is None else size
    return msc_data_group(dg_type, (((repetition_count & 7) << 13) | (size & 0x1FFF)).to_bytes(2, "big") + segment, tid,
                          (number, last), **kw)


def mot_object_groups(tid, header, body, seg_size, header_seg_size=None, **kw):
    """the data groups of one object in header mode: the header's segments (type 3), then the body's (type 4)"""
    out = []
    for dg_type, part, size in ((MOT_DG_HEADER, header, header_seg_size or max(len(header), 1)), (MOT_DG_BODY, body, seg_size)):
        segs = mot_segments(part, size)
        out += [mot_group(dg_type, tid, n, n == len(segs) - 1, seg, continuity=n, **kw) for n, seg in enumerate(segs)]
    return out


MOT_DG_DIRECTORY, MOT_DG_DIRECTORY_COMPRESSED = 6, 7


def mot_directory(objects, period=0, segment_size=0, extension=b"", compressed=False, size=None, count=None):
    """a MOT directory (EN 301 234 clause 7.2.2): CompressionFlag(1) Rfu(1) DirectorySize(30), NumberOfObjects(16),
    CarouselPeriod(24, tenths of a second; 0 = undefined), Rfu(1) Rfa(2) SegmentSize(13; 0 = not fixed),
    DirectoryExtensionLength(16), the directory extension, then per object its TransportId(16) and its MOT header (core and
    extension).  objects: [(transport id, header bytes)]; size / count: what the fields say (default: the truth);
    compressed sets the flag alone"""
    extension = bytes(extension)
    entries = b"".join(int(tid).to_bytes(2, "big") + bytes(header) for tid, header in objects)
    total = 13 + len(extension) + len(entries) if size is None else size
    n = len(objects) if count is None else count
    assert total < 1 << 30 and n < 1 << 16 and period < 1 << 24 and segment_size < 1 << 13 and len(extension) < 1 << 16
    return ((int(compressed) << 31) | total).to_bytes(4, "big") + n.to_bytes(2, "big") + period.to_bytes(3, "big") + \
        segment_size.to_bytes(2, "big") + len(extension).to_bytes(2, "big") + extension + entries


def mot_carousel_groups(dir_tid, objects, seg_size, dir_seg_size=None, period=0, extension=b"", **kw):
    """one cycle of a MOT directory carousel (EN 301 234 clause 7.2): objects is [(transport id, header, body)].  ->
    (the directory's data groups (type 6), [the body's data groups (type 4) of each object]); no header groups (type 3) are
    sent in directory mode: the headers travel in the directory.  dir_seg_size: default the whole directory in one segment"""
    directory = mot_directory([(tid, header) for tid, header, _ in objects], period, 0, extension)
    segs = mot_segments(directory, dir_seg_size or len(directory))
    dir_groups = [mot_group(MOT_DG_DIRECTORY, dir_tid, n, n == len(segs) - 1, seg, continuity=n, **kw) for n, seg in enumerate(segs)]
    bodies = []
    for tid, _, body in objects:
        segs = mot_segments(body, seg_size)
        bodies.append([mot_group(MOT_DG_BODY, tid, n, n == len(segs) - 1, seg, continuity=n, **kw) for n, seg in enumerate(segs)])
    return dir_groups, bodies


def dgli(length, good=True):
    """the data group length indicator: rfa(2) length(14), the CRC over these two bytes"""
    assert 0 <= length < 1 << 14
    b = bytes([length >> 8, length & 0xFF])
    c = crc16(b) ^ (0 if good else 0x0100)
    return b + bytes([c >> 8, c & 0xFF])


def mot_fields(groups, length_index, with_length=True, per_au=1):
    """-> per access unit the X-PAD sub-fields [(type, data)] that carry these data groups: in a group's first access unit
    the length indicator (type 1, 4 bytes) and a start sub-field (type 12), then continuation sub-fields (type 13), each
    of XPAD_LENGTHS[length_index] bytes, the last one filled up with zeros; per_au: sub-fields of a group per access unit
    (the length indicator counts as one)"""
    n, out = XPAD_LENGTHS[length_index], []
    for g in groups:
        g = bytes(g)
        subs = [(XPAD_DGLI, dgli(len(g)))] if with_length else []
        for k, at in enumerate(range(0, len(g), n)):
            part = g[at:at + n]
            subs.append((XPAD_MOT_CONT if k else XPAD_MOT_START, part + bytes(n - len(part))))
        if per_au == 1 and with_length:
            subs[:2] = [subs[:2]]                                        # (the indicator travels with the start sub-field)
            out += [f if isinstance(f, list) else [f] for f in subs]
        else:
            out += [subs[i:i + per_au] for i in range(0, len(subs), per_au)]
    return out


def merge_fields(*streams):
    """per access unit, the sub-fields of several applications side by side in one list, in the order given (a stream
    that has ended adds nothing)"""
    return [sum((list(s[k]) for s in streams if k < len(s)), []) for k in range(max(len(s) for s in streams))]


def dls_fields(groups, length_index):
    """dls_pads' sub-fields without their PAD: per access unit [(type, data)], for merge_fields"""
    return [[f] for g in groups for f in dls_subfields(g, [XPAD_LENGTHS[length_index]])]


def fields_pads(fields, ci_less=False, n=None, end_marker=True):
    """one variable X-PAD field per access unit from its sub-fields (at most four); None where there are none.  ci_less: an
    access unit with ONE sub-field of a continuation type (3, 13) that continues the last sub-field of the list before it,
    with the same length, goes without a list."""
    pads, prev = [], None
    for f in fields:
        if not f:
            pads.append(None)
            prev = None
            continue
        cont = {XPAD_DLS_START: XPAD_DLS_CONT, XPAD_DLS_CONT: XPAD_DLS_CONT, XPAD_MOT_START: XPAD_MOT_CONT, XPAD_MOT_CONT: XPAD_MOT_CONT}
        if ci_less and prev is not None and len(f) == 1 and f[0][0] == cont.get(prev[0]) and len(f[0][1]) == len(prev[1]):
            pads.append(pad_field(f[0][1], 2, 0, n))
        else:
            pads.append(pad_field(xpad_variable(f, end_marker), 2, 1, n))
        prev = f[-1]
    return pads


def mot_pads(groups, length_index, ci_less=False, before=(), after=(), n=None, with_length=True, end_marker=True, per_au=1):
    """One PAD field per access unit for a sequence of MOT data groups (mot_fields).  before / after: other applications'
    sub-fields around them in every list -- fixed [(type, data)], or per access unit (dls_fields(...): a label beside the
    slide); ci_less: the continuation sub-fields go without a list where they stand alone."""
    own = mot_fields(groups, length_index, with_length, per_au)
    side = lambda f: [list(f)] * len(own) if (not f or isinstance(f[0], tuple)) else [list(x) for x in f]
    return fields_pads(merge_fields(side(before), own, side(after)), ci_less, n, end_marker)


def pack_pads(sizes, mot_groups, dls_groups, dls_index=0):
    """One PAD per access unit, as large as the unit has room for: a label sub-field of XPAD_LENGTHS[dls_index] bytes in front while the label
    lasts, then the length indicator and sub-fields of the slide's current data group, the largest that fit.
    sizes: bytes of every access unit with its CRC -> PAD per unit (None: no room), sub-fields left over"""
    mot = [bytes(g) for g in mot_groups]
    dls = [f[0] for f in dls_fields(dls_groups, dls_index)]
    pads, at = [], 0                                                  # at: bytes of mot[0] already sent
    for size in sizes:
        room = min(size - 2 - 3 - 2 - 4, 190)                         # CRC, element header, F-PAD, content indicators
        fields = []
        if dls and room >= XPAD_LENGTHS[dls_index]:
            fields.append(dls.pop(0))
            room -= XPAD_LENGTHS[dls_index]
        if mot and at == 0 and room >= 8 and len(fields) <= 2:
            fields.append((XPAD_DGLI, dgli(len(mot[0]))))
            room -= 4
        while mot and len(fields) < 4 and room >= 4 and (at > 0 or (fields and fields[-1][0] == XPAD_DGLI)):
            left = len(mot[0]) - at
            fit = [n for n in XPAD_LENGTHS if n <= room]
            n = min([m for m in fit if m >= left] or [fit[-1]])
            part = mot[0][at:at + n]
            fields.append((XPAD_MOT_CONT if at else XPAD_MOT_START, part + bytes(n - len(part))))
            room -= n
            at += n
            if at >= len(mot[0]):
                mot.pop(0)
                at = 0
                break
        pads.append(pad_field(xpad_variable(fields), 2, 1) if fields else None)
    return pads, len(mot) + len(dls)


# ----------------------------------------------------------------------------- FIGs (EN 300 401 clauses 5.2, 6, 8)
# Packet mode (EN 300 401 clause 5.3.2): a sub-channel of bit rate R carries logical frames of R / 8 slots of 24 bytes;
# a packet is 1 .. 4 slots: length (2 bits) continuity index (2) first (1) last (1) address (10) command (1) useful data
# length (7), the data field (useful bytes, then padding), the CRC (the FIB's, big-endian).  Data groups (msc_data_group)
# travel cut into the useful bytes of packets of one address.
PACKET_SLOT = 24
PACKET_FEC_ADDRESS = 1022
DSCTY_MOT = 60


def packet(address, data, slots=None, ci=0, first=True, last=True, command=False, crc=True, udl=None, fill=0):
    """one packet: slots (default: as few as hold the data) * 24 bytes; crc=False sends a wrong CRC; udl: what the header
    says (default: the truth)"""
    data = bytes(data)
    if slots is None:
        slots = max(1, -(-(len(data) + 5) // PACKET_SLOT))
    room = PACKET_SLOT * slots - 5
    assert 1 <= slots <= 4 and len(data) <= room and 0 <= address < 1024
    n = len(data) if udl is None else udl
    head = _bits((slots - 1, 2), (ci & 3, 2), (int(first), 1), (int(last), 1), (address, 10), (int(command), 1), (n, 7))
    body = head + data + bytes([fill]) * (room - len(data))
    c = crc16(body) ^ (0 if crc else 0x0040)
    return body + bytes([c >> 8, c & 0xFF])


def packetise(groups, address, sizes=(4,), ci=0):
    """data groups -> packets of one address, continuity index from `ci`: each group in packets of sizes[k % len] slots
    (k: the running packet number), the last one of a group as short as holds the rest; an empty group is one packet"""
    out, k = [], 0
    for g in groups:
        g, at = bytes(g), 0
        while True:
            room = PACKET_SLOT * sizes[k % len(sizes)] - 5
            rest = len(g) - at
            final = rest <= room
            take = rest if final else room
            out.append(packet(address, g[at:at + take], None if final else sizes[k % len(sizes)], ci=ci + k, first=at == 0, last=final))
            k += 1
            at += take
            if final:
                break
    return out


def wrong_crc(group):
    """a data group that carries a CRC (msc_data_group(..., crc=True)), with that CRC wrong"""
    g = bytearray(group)
    g[-1] ^= 0x01
    return bytes(g)


def packetise_chosen(group, address, plan, ci=0):
    """one data group in packets of chosen shape: plan is a list of (slots, udl) -- that many slots, the next udl bytes of
    the group (0 included; less than the room is filled up) -- and of ("command", slots) for a command packet between them;
    the plan must take the group exactly.  First is set on the first data packet, last on the last.  -> packets (continuity
    index from `ci`, counting command packets too)"""
    group, at, out = bytes(group), 0, []
    data_items = [i for i, p in enumerate(plan) if p[0] != "command"]
    assert sum(plan[i][1] for i in data_items) == len(group) and data_items
    for i, p in enumerate(plan):
        if p[0] == "command":
            out.append(packet(address, b"\xC3" * 3, p[1], ci=ci + i, first=True, last=True, command=True))
            continue
        slots, udl = p
        out.append(packet(address, group[at:at + udl], slots, ci=ci + i, first=i == data_items[0], last=i == data_items[-1], fill=0xEE))
        at += udl
    return out


def packetise_raw(data, address, sizes=(4,), ci=0, flags=((True, True), (False, False), (True, False), (False, True))):
    """a byte string for a component without data groups (DG flag 1): packets of sizes[k % len] slots, each full but the last;
    first and last take flags[k % len] (a receiver must not look at them)"""
    data, at, out, k = bytes(data), 0, [], 0
    while at < len(data) or k == 0:
        slots = sizes[k % len(sizes)]
        take = min(PACKET_SLOT * slots - 5, len(data) - at)
        first, last = flags[k % len(flags)]
        out.append(packet(address, data[at:at + take], slots, ci=ci + k, first=first, last=last, fill=0xEE))
        at += take
        k += 1
    return out


def padding_packet(slots=1, fill=0x55):
    """a padding packet: address 0, no useful data"""
    return packet(0, b"", slots, fill=fill)


def fec_packet(rng):
    """24 bytes shaped like an FEC packet: one slot, address 1022, the other 21 bytes what RS parity would be (random): no
    packet CRC"""
    return _bits((0, 2), (int(rng.integers(0, 4)), 2), (0, 1), (0, 1), (PACKET_FEC_ADDRESS, 10)) + bytes(rng.integers(0, 256, 22, dtype=np.uint8))


def packet_frames(bitrate, streams, n_frames=None):
    """logical frames [n][3 * bitrate] uint8 of a packet-mode sub-channel: streams is a list of packet lists; a frame takes the
    next packet of each stream in turn while it fits (a packet never straddles frames; order within a stream is kept), the
    rest of the frame is padding packets.  n_frames: at least that many frames (of padding, behind the streams)"""
    slots = bitrate // 8
    assert bitrate % 8 == 0 and 1 <= slots <= 64
    queues = [list(q) for q in streams]
    assert all(len(p) % PACKET_SLOT == 0 and len(p) // PACKET_SLOT <= slots for q in queues for p in q)
    frames = []
    while any(queues) or len(frames) < (n_frames or 0):
        frame, blocked = b"", [False] * len(queues)
        while True:
            moved = False
            for i, q in enumerate(queues):
                if q and not blocked[i]:
                    if len(frame) + len(q[0]) <= PACKET_SLOT * slots:
                        frame += q.pop(0)
                        moved = True
                    else:
                        blocked[i] = True
            if not moved:
                break
        while len(frame) < PACKET_SLOT * slots:
            frame += padding_packet(min(4, slots - len(frame) // PACKET_SLOT))
        frames.append(np.frombuffer(frame, np.uint8))
    return np.stack(frames) if frames else np.zeros((0, 3 * bitrate), np.uint8)


# FEC for packet mode (EN 300 401 clause 5.3.5): an FEC frame is 94 slots of packets (the application data table, 2256 bytes
# filled column by column into 12 rows of 188) followed by nine FEC packets: length 0, counter 0..8 (4 bits), address 1022,
# then 22 bytes of the RS data table (12 rows of 16 parity bytes, read column by column; the last six bytes are padding).
PACKET_FEC_DATA_SLOTS = 94
PACKET_FEC_SLOTS = 9


def _rs204_generator():
    g = [1]                                   # g[i] = coefficient of x^i
    for k in range(16):
        nx = [0] * (len(g) + 1)
        for i, c in enumerate(g):
            nx[i + 1] ^= c
            nx[i] ^= _gf_mul(c, int(_GF_EXP[k]))
        g = nx
    return g


_RS204_G = _rs204_generator()


def rs204_parity(row188):
    """RS(204,188) parity, 16 bytes: the remainder of d(x) x^16 by prod_{k=0..15}(x - alpha^k), GF(2^8) / 0x11D, the first
    byte the highest degree (RS(255,239) shortened by 51 leading zeros)."""
    assert len(row188) == 188
    rem = [0] * 16                            # rem[0] = highest degree
    for d in row188:
        fb = int(d) ^ rem[0]
        rem = [rem[j + 1] ^ _gf_mul(fb, _RS204_G[15 - j]) for j in range(15)] + [_gf_mul(fb, _RS204_G[0])]
    return np.array(rem, np.uint8)


def fec_frame(packets):
    """94 slots of packets (a list of packets, or their 2256 bytes) -> the 103 slots of an FEC frame, as bytes: the packets
    as they are, then the nine FEC packets with counters 0..8"""
    data = packets if isinstance(packets, (bytes, bytearray)) else b"".join(bytes(p) for p in packets)
    assert len(data) == PACKET_SLOT * PACKET_FEC_DATA_SLOTS
    table = np.frombuffer(bytes(data), np.uint8).reshape(188, 12)         # [column][row]
    parity = np.stack([rs204_parity(table[:, r]) for r in range(12)])     # [row][16]
    rs = parity.T.tobytes() + bytes(6)                                     # column by column, 192 bytes, then padding
    out = bytes(data)
    for c in range(PACKET_FEC_SLOTS):
        out += _bits((0, 2), (c, 4), (PACKET_FEC_ADDRESS, 10)) + rs[22 * c:22 * c + 22]
    return out


def packet_fec_frames(bitrate, streams, n_frames=None):
    """logical frames [n][3 * bitrate] uint8 of an FEC-protected packet-mode sub-channel (FEC scheme 1): streams is a list of
    packet lists, taken a packet of each in turn; no packet straddles a logical frame or the 94-slot application data table
    (padding packets fill up to either), and every full table is followed by its nine FEC packets.  The first table begins
    with the first frame.  n_frames: at least that many frames (padding and FEC packets behind the streams); the last table
    may be left unfinished"""
    slots = bitrate // 8
    assert bitrate % 8 == 0 and 1 <= slots <= 64
    queues = [list(q) for q in streams]
    assert all(len(p) % PACKET_SLOT == 0 and len(p) // PACKET_SLOT <= slots for q in queues for p in q)
    out, table, turn = b"", b"", 0

    def put(p):
        nonlocal out, table
        out += p
        table += p
        if len(table) == PACKET_SLOT * PACKET_FEC_DATA_SLOTS:
            out += fec_frame(table)[len(table):]
            table = b""

    while any(queues) or len(out) % (PACKET_SLOT * slots) or len(out) < (n_frames or 0) * PACKET_SLOT * slots:
        room = min(slots - len(out) // PACKET_SLOT % slots, PACKET_FEC_DATA_SLOTS - len(table) // PACKET_SLOT)
        nxt = None
        if any(queues):
            while not queues[turn % len(queues)]:
                turn += 1
            nxt = queues[turn % len(queues)]
        if nxt and len(nxt[0]) // PACKET_SLOT <= room:
            put(nxt.pop(0))
            turn += 1
        else:
            put(padding_packet(min(4, room)))
    return np.frombuffer(out, np.uint8).reshape(-1, PACKET_SLOT * slots).copy()


# What a multiplex says about itself in the FIC: enough for a receiver to find and decode its audio services
# without being told anything (FIG 0/0 ensemble, 0/1 sub-channel organisation, 0/2 service organisation,
# 1/0 ensemble label, 1/1 service labels).
ASCTY_DAB = 0          # MPEG-1/2 layer II
ASCTY_DABPLUS = 63     # HE-AAC v2 super-frames (TS 102 563)


def _bits(*fields):
    """fields: (value, width) ... MSB first -> bytes (total width must be a multiple of 8)."""
    v, n = 0, 0
    for val, w in fields:
        assert 0 <= val < (1 << w), (val, w)
        v = (v << w) | val
        n += w
    assert n % 8 == 0
    return bytes((v >> (8 * (n // 8 - 1 - i))) & 0xFF for i in range(n // 8))


def fig0(ext, body, cn=0, oe=0, pd=0):
    data = _bits((cn, 1), (oe, 1), (pd, 1), (ext, 5)) + body
    assert len(data) <= 29
    return _bits((0, 3), (len(data), 5)) + data


def fig0_0(eid, cif_count, change=0, alarm=0):
    return fig0(0, _bits((eid, 16), (change, 2), (alarm, 1), ((cif_count // 250) % 20, 5), (cif_count % 250, 8)))


def fig0_1(subchannels):
    """subchannels: dicts {id, start, option, level, size} (long form, EEP) or {id, start, uep_index} (short form)."""
    body = b""
    for sc in subchannels:
        if "uep_index" in sc:
            body += _bits((sc["id"], 6), (sc["start"], 10), (0, 1), (0, 1), (sc["uep_index"], 6))
        else:
            body += _bits((sc["id"], 6), (sc["start"], 10), (1, 1), (sc["option"], 3), (sc["level"] - 1, 2), (sc["size"], 10))
    return fig0(1, body)


def fig0_2(services, pd=0):
    """services: dicts {sid (16 bit; 32 with pd=1), components: [{subchannel, ascty, primary}]} (MSC stream audio) or
    [{scid, primary}] (packet mode, TMId 3: the 12-bit service component identifier FIG 0/3 describes)."""
    body = b""
    for sv in services:
        comps = sv["components"]
        body += _bits((sv["sid"], 32 if pd else 16), (0, 1), (0, 3), (len(comps), 4))
        for c in comps:
            if "scid" in c:
                body += _bits((3, 2), (c["scid"], 12), (1 if c.get("primary", True) else 0, 1), (0, 1))
            else:
                body += _bits((0, 2), (c["ascty"], 6), (c["subchannel"], 6), (1 if c.get("primary", True) else 0, 1), (0, 1))
    return fig0(2, body, pd=pd)


def fig0_3(entries):
    """Service component in packet mode (clause 6.3.2): dicts {scid, subchannel, address, dscty (default 60, MOT), dg_flag
    (default 0: data groups are used), caorg (default None: no CAOrg field)}."""
    body = b""
    for e in entries:
        caorg = e.get("caorg")
        body += _bits((e["scid"], 12), (0, 3), (0 if caorg is None else 1, 1), (e.get("dg_flag", 0), 1), (0, 1), (e.get("dscty", DSCTY_MOT), 6),
                      (e["subchannel"], 6), (e["address"], 10))
        if caorg is not None:
            body += _bits((caorg, 16))
    return fig0(3, body)


def fig0_14(entries):
    """FEC sub-channel organisation (clause 6.2.2): [(subchannel_id, fec_scheme), ...]."""
    return fig0(14, b"".join(_bits((scid, 6), (fec, 2)) for scid, fec in entries))


def fig0_5(entries):
    """Service component language, short form: [(subchannel_id, language), ...] (clause 8.1.2)."""
    return fig0(5, b"".join(_bits((0, 1), (0, 1), (scid, 6), (lang, 8)) for scid, lang in entries))


def fig0_6(lsn, ids, idlq=0, active=1, hard=1, ils=0, pd=0):
    """Service linking (clause 8.1.15): one linkage set with an id list.  idlq 0 = DAB SIds, 1 = RDS PI codes,
    3 = DRM service ids; ils = 1: every id is (ECC, id) given as a 24-bit number; pd = 1: 32-bit SIds."""
    width = 32 if pd else (24 if ils else 16)
    body = _bits((1, 1), (active, 1), (hard, 1), (ils, 1), (lsn, 12), (0, 1), (idlq, 2), (0, 1), (len(ids), 4))
    body += b"".join(_bits((i, width)) for i in ids)
    return fig0(6, body, pd=pd)


def fig0_8(entries, pd=0):
    """Service component global definition, short form: [(sid, scids, subchannel_id), ...] (clause 6.3.5)."""
    w = 32 if pd else 16
    return fig0(8, b"".join(_bits((sid, w), (0, 1), (0, 3), (scids, 4), (0, 1), (0, 1), (scid, 6)) for sid, scids, scid in entries), pd=pd)


def fig0_8_long(entries, pd=0):
    """Service component global definition, long form (packet mode): [(sid, scids, scid 12 bits), ...] (clause 6.3.5)."""
    w = 32 if pd else 16
    return fig0(8, b"".join(_bits((sid, w), (0, 1), (0, 3), (scids, 4), (1, 1), (0, 3), (scid, 12)) for sid, scids, scid in entries), pd=pd)


def fig0_13(entries, pd=0):
    """User application information (clause 6.3.6): [(sid, scids, [(ua_type 11 bits, data bytes), ...]), ...]."""
    w = 32 if pd else 16
    body = b""
    for sid, scids, apps in entries:
        body += _bits((sid, w), (scids, 4), (len(apps), 4))
        for ua_type, data in apps:
            assert len(data) < 32
            body += _bits((ua_type, 11), (len(data), 5)) + bytes(data)
    return fig0(13, body, pd=pd)


def fig0_9(ecc, lto_half_hours, inter_table=1):
    """Country, LTO and international table (clause 8.1.3.2); lto in half hours, negative = west of UTC."""
    return fig0(9, _bits((0, 1), (0, 1), (1 if lto_half_hours < 0 else 0, 1), (abs(lto_half_hours), 5), (ecc, 8), (inter_table, 8)))


def fig0_17(entries):
    """Programme type: [(sid, int_code, language or None), ...] (clause 8.1.5)."""
    body = b""
    for sid, code, lang in entries:
        body += _bits((sid, 16), (0, 1), (0, 1), (0 if lang is None else 1, 1), (0, 1), (0, 4))
        if lang is not None:
            body += _bits((lang, 8))
        body += _bits((0, 3), (code, 5))
    return fig0(17, body)


def fig0_21(entries, oe=0):
    """Frequency information (clause 8.1.8), one block: entries [(id, rm, continuity, frequencies in Hz), ...] with
    rm 0 = DAB ensemble (16 kHz steps), 8 = FM with RDS (87.5 MHz + 100 kHz steps), 6 = DRM (id is 24 bits, kHz)."""
    blk = b""
    for ident, rm, cont, freqs in entries:
        if rm == 0:
            fl = b"".join(_bits((0, 5), (f // 16000, 19)) for f in freqs)
        elif rm == 8:
            fl = bytes((f - 87500000) // 100000 for f in freqs)
        else:
            fl = bytes([ident >> 16]) + b"".join(_bits((0, 1), (f // 1000, 15)) for f in freqs)
        assert len(fl) <= 7
        blk += _bits((ident & 0xFFFF, 16), (rm, 4), (cont, 1), (len(fl), 3)) + fl
    return fig0(21, _bits((0, 11), (len(blk), 5)) + blk, oe=oe)


def fig0_24(entries, pd=0):
    """Services in other ensembles: [(sid, [eid, ...]), ...] (clause 8.1.10.2)."""
    w = 32 if pd else 16
    return fig0(24, b"".join(_bits((sid, w), (0, 1), (0, 3), (len(eids), 4)) + b"".join(_bits((e, 16)) for e in eids)
                             for sid, eids in entries), pd=pd, oe=1)


def fig1_4(sid, scids, label, pd=0, charset=0):
    """Service component label (clause 8.1.14.3)."""
    text = label.encode("latin-1")[:16].ljust(16, b" ")
    data = _bits((charset, 4), (0, 1), (4, 3), (pd, 1), (0, 3), (scids, 4), (sid, 32 if pd else 16)) + text + _bits((0xFF00, 16))
    return _bits((1, 3), (len(data), 5)) + data


def fig1_5(sid32, label, charset=0):
    """Data service label: 32-bit service identifier (clause 8.1.14.2)."""
    text = label.encode("latin-1")[:16].ljust(16, b" ")
    data = _bits((charset, 4), (0, 1), (5, 3), (sid32, 32)) + text + _bits((0xFF00, 16))
    return _bits((1, 3), (len(data), 5)) + data


def mjd(year, month, day):
    """Modified Julian date of a calendar date (inverse of the standard's annex formula)."""
    a = (14 - month) // 12
    y, m = year + 4800 - a, month + 12 * a - 3
    jdn = day + (153 * m + 2) // 5 + 365 * y + y // 4 - y // 100 + y // 400 - 32045
    return jdn - 2400001


def fig0_10(year, month, day, hours, minutes, seconds=None, milliseconds=0):
    """Date and time (clause 8.1.3.1): short form without seconds, long form with seconds and milliseconds."""
    long_form = seconds is not None
    body = _bits((0, 1), (mjd(year, month, day), 17), (0, 1), (0, 1), (1 if long_form else 0, 1), (hours, 5), (minutes, 6))
    if long_form:
        body += _bits((seconds, 6), (milliseconds, 10))
    return fig0(10, body)


def fig1(ext, ident, label, charset=0):
    text = label.encode("latin-1")[:16].ljust(16, b" ")
    data = _bits((charset, 4), (0, 1), (ext, 3), (ident, 16)) + text + _bits((0xFF00, 16))
    return _bits((1, 3), (len(data), 5)) + data


def pack_fibs(figs):
    """Greedy packing of FIGs (bytes) into 30-byte FIB data fields (end marker 0xFF, zero padding) + CRC."""
    fibs, cur = [], b""
    for f in figs:
        assert len(f) <= 30
        if len(cur) + len(f) > 30:
            fibs.append(cur)
            cur = b""
        cur += f
    if cur:
        fibs.append(cur)
    out = np.zeros((len(fibs), 32), np.uint8)
    for i, d in enumerate(fibs):
        d = d + (b"\xff" if len(d) < 30 else b"")
        d = d.ljust(30, b"\x00")
        c = crc16(d)
        out[i] = np.frombuffer(d + bytes([c >> 8, c & 0xFF]), np.uint8)
    return out


class ServiceEnsemble:
    """A cyclic multiplex that describes itself: DAB+ services on EEP sub-channels carrying real super-frames,
    FIC made of FIG 0/0, 0/1, 0/2, 1/0, 1/1.  services = [(label, sid, subchannel_id, option, level, bitrate,
    start_cu), ...].  n_frames must be a multiple of 5 so that whole super-frames (5 logical frames) tile."""

    def __init__(self, seed, services, n_frames=5, eid=0xC181, label="Synth Ensemble", dab_services=(), extras=True, bodies=None,
                 dab_pads=None, packet_services=(), user_applications=()):
        """dab_services: DAB (MPEG layer II) services on UEP sub-channels, [(label, sid, subchannel_id, uep_index,
        start_cu), ...]; every logical frame of such a sub-channel is one layer-II frame (header + random body).
        extras=False leaves the rotation to the labels alone (FIG 0/0, 0/1, 0/2, 0/10 and one label per CIF): what
        four services leave room for in three FIBs.
        bodies: per DAB+ service (or None), per super-frame, build_superframe's `bodies`: what the access units begin
        with (PAD); the random draws do not depend on it.
        dab_pads: per DAB service (or None), per logical frame, the PAD (pad_field's bytes, or None: F-PAD alone) of that frame: the
        service then sends mp2_frame()s with the ISO CRC, 48 kHz (stereo, or single channel at the rates only that mode may
        use), from a generator of their own; the draws of everything else do not depend on it.
        packet_services: packet-mode data services on EEP sub-channels, [(label, sid, subchannel_id, option, level, bitrate,
        start_cu, components, frames, fec_scheme), ...]: components = [(scid, packet address, dscty, dg_flag), ...] (FIG 0/2
        TMId 3 and FIG 0/3; the first is the primary one), frames = 4 * n_frames logical frames (packet_frames), fec_scheme
        non-zero announces FIG 0/14.  No random draw depends on them.
        user_applications: of packet-mode components, [(sid, scids, scid, [(ua_type, data), ...]), ...]: one FIG 0/8 (long form)
        and one FIG 0/13 for all of them, in rotation with the labels."""
        assert n_frames % 5 == 0
        rng = np.random.default_rng(seed)
        self.n_frames, self.eid, self.label, self.services = n_frames, eid, label, services
        R = 4 * n_frames
        cifs = rng.integers(0, 2, size=(R, NB_CIF_BITS), dtype=np.uint8)
        self.masks, self.sizes, self.msc_bytes, self.superframes, self.aus = [], [], [], [], []
        self.subchannels = []
        for n_sv, (lab, sid, scid, option, level, bitrate, start_cu) in enumerate(services):
            mask, size_cu = eep_mask(option, level, bitrate)
            sfs, aus = [], []
            for q in range(R // 5):
                sf, starts, au = build_superframe(rng, bitrate, dac_rate=1, sbr=1, channel_mode=1, ps=0,
                                                  bodies=bodies[n_sv][q] if bodies is not None and bodies[n_sv] is not None else None)
                sfs.append(sf); aus.append(au)
            data = np.concatenate(sfs).reshape(R, bitrate * 3)
            coded = np.stack([msc_encode_lf(data[r], mask) for r in range(R)])
            cifs[:, start_cu * 64:(start_cu + size_cu) * 64] = time_interleave(coded, cyclic=True)
            self.masks.append(mask); self.sizes.append(size_cu); self.msc_bytes.append(data)
            self.superframes.append(sfs); self.aus.append(aus)
            self.subchannels.append({"id": scid, "start": start_cu, "option": option, "level": level, "size": size_cu})
        self.dab_services, self.mp2_frames = list(dab_services), []
        for (lab, sid, scid, uidx, start_cu) in self.dab_services:
            mask, size_cu = uep_mask(uidx)
            bitrate = _UEP_TABLE[uidx][0]
            data = rng.integers(0, 256, size=(R, bitrate * 3), dtype=np.uint8)
            data[:, 0], data[:, 1] = 0xFF, 0xFD                     # sync, MPEG-1, layer II, no CRC
            data[:, 2] = (data[:, 2] & 0xF0) | 0x04                 # 48 kHz
            data[:, 3] &= 0x3F                                      # stereo
            if dab_pads is not None and dab_pads[len(self.mp2_frames)] is not None:
                pads, frng = dab_pads[len(self.mp2_frames)], np.random.default_rng([seed, scid])
                mode = MP2_MONO if bitrate in (32, 48, 56, 80) else MP2_STEREO
                data = np.stack([mp2_frame(frng, bitrate, mode=mode, pad=pads[r] if r < len(pads) and pads[r] is not None else bytes(2))
                                 for r in range(R)])
            coded = np.stack([msc_encode_lf(data[r], mask) for r in range(R)])
            coded = np.concatenate([coded, np.zeros((R, size_cu * 64 - coded.shape[1]), np.uint8)], axis=1)
            cifs[:, start_cu * 64:(start_cu + size_cu) * 64] = time_interleave(coded, cyclic=True)
            self.mp2_frames.append(data)
            self.subchannels.append({"id": scid, "start": start_cu, "uep_index": uidx})
        self.packet_services = list(packet_services)
        packet_figs = []
        for (lab, sid, scid, option, level, bitrate, start_cu, comps, frames, fec) in self.packet_services:
            mask, size_cu = eep_mask(option, level, bitrate)
            data = np.ascontiguousarray(frames, np.uint8)
            assert data.shape == (R, bitrate * 3), (data.shape, R, bitrate)
            coded = np.stack([msc_encode_lf(data[r], mask) for r in range(R)])
            cifs[:, start_cu * 64:(start_cu + size_cu) * 64] = time_interleave(coded, cyclic=True)
            self.subchannels.append({"id": scid, "start": start_cu, "option": option, "level": level, "size": size_cu})
            packet_figs.append(fig0_3([{"scid": c[0], "subchannel": scid, "address": c[1], "dscty": c[2], "dg_flag": c[3]} for c in comps]))
            if fec:
                packet_figs.append(fig0_14([(scid, fec)]))
        sv = [{"sid": sid, "components": [{"subchannel": scid, "ascty": ASCTY_DABPLUS}]}
              for (lab, sid, scid, *_rest) in services]
        sv += [{"sid": sid, "components": [{"subchannel": scid, "ascty": ASCTY_DAB}]}
               for (lab, sid, scid, *_rest) in self.dab_services]
        labels = [fig1(0, eid, label)] + [fig1(1, sid, lab) for (lab, sid, *_rest) in services]
        labels += [fig1(1, sid, lab) for (lab, sid, *_rest) in self.dab_services]
        sv += [{"sid": sid, "components": [{"scid": c[0], "primary": k == 0} for k, c in enumerate(comps)]}
               for (lab, sid, _scid, _o, _l, _b, _s, comps, *_rest) in self.packet_services]
        labels += [fig1(1, sid, lab) for (lab, sid, *_rest) in self.packet_services]
        if user_applications:
            labels += [fig0_8_long([(sid, scids, scid) for (sid, scids, scid, _a) in user_applications]),
                       fig0_13([(sid, scids, apps) for (sid, scids, _c, apps) in user_applications])]
        # what else a multiplex says about itself (one of these per CIF, in rotation with the labels): country and
        # local time, component identifiers and labels, programme types, languages, a linkage set with its FM
        # alternative and that station's frequencies, the neighbouring ensemble carrying the first service
        all_sv = [(lab, sid, scid) for (lab, sid, scid, *_r) in services] + [(lab, sid, scid) for (lab, sid, scid, *_r) in self.dab_services]
        first_sid = all_sv[0][1]
        if extras:
            labels += [fig0_9(0xE1, 2, 1),
                       fig0_8([(sid, 0, scid) for (_l, sid, scid) in all_sv[:5]]),
                       fig0_17([(sid, 1 + k % 30, 0x09 if k == 0 else None) for k, (_l, sid, _s) in enumerate(all_sv[:5])]),
                       fig0_5([(scid, 0x09 + k) for k, (_l, _sid, scid) in enumerate(all_sv[:8])]),
                       fig0_6(0x123, [first_sid], idlq=0), fig0_6(0x123, [0xC479], idlq=1),
                       fig0_21([(0xC479, 8, 1, [98300000, 101100000]), (0xC182, 0, 0, [225648000])]),
                       fig0_24([(first_sid, [0xC182])])]
            labels += [fig1_4(sid, 0, (lab + " main")[:16]) for (lab, sid, _s) in all_sv[:3]]
        self.fibs = np.zeros((n_frames, 12, 32), np.uint8)
        k = 0
        for f in range(n_frames):
            for c in range(4):
                figs = [fig0_0(eid, 4 * f + c)]
                figs += [fig0_1(self.subchannels[i:i + 6]) for i in range(0, len(self.subchannels), 6)]
                figs += [fig0_2(sv[i:i + 5]) for i in range(0, len(sv), 5)]
                figs += packet_figs
                figs.append(labels[k % len(labels)]); k += 1
                if c == 3:                                    # once per frame: date and time, advancing 96 ms
                    ms = 96 * f
                    figs.append(fig0_10(2024, 2, 29, 23, 59, 58 + ms // 1000 if ms < 2000 else 59, ms % 1000))
                fibs = pack_fibs(figs)
                assert len(fibs) <= 3, "too many FIGs for one CIF's three FIBs"
                pad = pack_fibs([fig0_0(eid, 4 * f + c)])
                block = np.concatenate([fibs] + [pad] * (3 - len(fibs)))
                self.fibs[f, 3 * c:3 * c + 3] = block
        self.frame_bits = np.zeros((n_frames, NB_FRAME_BITS), np.uint8)
        for f in range(n_frames):
            self.frame_bits[f, :NB_FIC_BITS] = fic_encode(self.fibs[f])
            self.frame_bits[f, NB_FIC_BITS:] = cifs[4 * f:4 * f + 4].ravel()

    def iq(self):
        return np.stack([modulate_frame(self.frame_bits[f]) for f in range(self.n_frames)])
