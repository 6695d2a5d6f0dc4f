"""dabgpu_dabplus_superframes and its _dev form bit for bit against the from-definition reference (dabplus_reference):
output bytes and the whole status record, at every bitrate, at the RS decoder's edges and beyond its reach (forced
miscorrections), at AU lengths across every multiple of 64, with broken headers, through every entry path and layout.
CPU: the reference equals the CPU oracle on every case built here."""
import functools

import numpy as np
import pytest

import dabplus_reference as R
from oracle import oracle as O

COMBOS = [(0, 1), (1, 1), (0, 0), (1, 0)]                 # (dac_rate, sbr): 2, 3, 4, 6 access units


# ---------------------------------------------------------------------------------------------------- building cases
def draw_starts(rng, s, n):
    """AU boundaries [first, c_1 .. c_{n-1}, 110 s]: gaps >= 3, starts <= 4095 (12-bit header fields)."""
    first, size = R.FIRST_START[n], 110 * s
    hi = min(size - 3, 4095)
    u = np.sort(rng.choice(hi - first - 3 - 2 * (n - 2) + 1, n - 1, replace=False))
    return [first] + [int(first + 3 + v + 2 * k) for k, v in enumerate(u)] + [size]


def data_part(rng, s, dac_rate, sbr, starts=None):
    """The 110 s data bytes of a super-frame: random bytes, every AU with valid bounds filled with a random payload and its
    CRC, then the header -- byte 2 (other bits random), the 12-bit starts (spare bits random), the Fire code."""
    n = R.num_aus(dac_rate, sbr)
    if starts is None:
        starts = draw_starts(rng, s, n)
    assert len(starts) == n + 1 and starts[n] == 110 * s and all(0 <= v < 4096 for v in starts[1:n])
    d = rng.integers(0, 256, 110 * s, dtype=np.uint8)
    for a in range(n):
        b0, b1 = starts[a], starts[a + 1]
        if b0 >= 3 and b1 <= 110 * s and b1 - b0 >= 3:
            c = R.au_crc(d[b0:b1 - 2])
            d[b1 - 2], d[b1 - 1] = c >> 8, c & 0xFF
    d[2] = (int(rng.integers(0, 256)) & 0x9F) | (dac_rate << 6) | (sbr << 5)
    bits = np.unpackbits(d[3:11])
    for a in range(1, n):
        bits[12 * (a - 1):12 * a] = [(starts[a] >> (11 - b)) & 1 for b in range(12)]
    d[3:11] = np.packbits(bits)
    fc = R.firecode(d[2:11])
    d[0], d[1] = fc >> 8, fc & 0xFF
    return d


def encode(data, s):
    """[n][110 s] data parts -> [n][120 s] super-frames: RS parity of each byte-interleaved column (reference encoder)."""
    data = np.asarray(data, np.uint8)
    n = data.shape[0]
    cols = data.reshape(n, R.K, s).transpose(0, 2, 1)
    return np.ascontiguousarray(R.rs_encode(cols).transpose(0, 2, 1)).reshape(n, 120 * s)


def hit_column(sf, s, j, rng, kind):
    """Damage column j of a super-frame in place."""
    col = sf[j::s].copy()
    if kind == "ff":
        col[:] = 0xFF
    elif kind == "zero":
        col[:] = 0
    elif kind == "mis":
        col = R.forced_miscorrection(col, rng)[0]
    else:
        pos = kind if isinstance(kind, list) else rng.choice(R.N, int(kind), replace=False)
        col[pos] ^= rng.integers(1, 256, len(pos), dtype=np.uint8)
    sf[j::s] = col


@functools.lru_cache(maxsize=None)
def rs_cases():
    """[(s, sfs)]: every column carries one of the edge patterns (0..5 errors), 6..10 random errors, a forced
    miscorrection, all 0xFF or all zero."""
    kinds = [list(p) for p in R.EDGE_ERROR_POSITIONS] + [6, 7, 8, 10, "mis", "mis", "mis", "ff", "zero"]
    out = []
    for s, nsf, seed in ((24, 12, 30), (5, 16, 31), (64, 3, 32)):
        rng = np.random.default_rng(seed)
        sfs = encode([data_part(rng, s, *COMBOS[f % 4]) for f in range(nsf)], s)
        for f in range(nsf):
            for j in range(s):
                hit_column(sfs[f], s, j, rng, kinds[int(rng.integers(0, len(kinds)))])
        out.append((s, sfs))
    return out


@functools.lru_cache(maxsize=None)
def bitrate_cases():
    """[(s, sfs)] for s = 1..64, two super-frames each, errors in every column: 1..5 in the first, 1..9 in the second."""
    out = []
    for s in range(1, 65):
        rng = np.random.default_rng(100 + s)
        sfs = encode([data_part(rng, s, *COMBOS[s % 4]), data_part(rng, s, *COMBOS[(s + 1) % 4])], s)
        for j in range(s):
            hit_column(sfs[0], s, j, rng, int(rng.integers(1, 6)))
            hit_column(sfs[1], s, j, rng, j % 9 + 1)
        out.append((s, sfs))
    return out


def crc_lengths():
    """AU payload lengths: 1..260, 64 k - 1, 64 k, 64 k + 1 up to the longest AU at s = 64 (7030: two AUs, the first of
    one byte), and that longest one."""
    longest = 110 * 64 - 5 - 3 - 2
    ls = set(range(1, 261)) | {64 * k + d for k in range(1, 111) for d in (-1, 0, 1)} | {longest}
    return sorted(v for v in ls if v <= longest)


@functools.lru_cache(maxsize=None)
def crc_cases():
    """-> (sfs [n][7680] at s = 64, expected au_crc_mask per super-frame).  Each length comes clean and with one bit wrong in
    its first payload byte, its last payload byte, each CRC byte; the RS parity is computed after the damage, so only the CRC
    can see it.  Units up to 4082 bytes are packed five to a six-AU super-frame (a clean filler last), longer ones are the
    second unit of a two-AU super-frame."""
    s, size = 64, 110 * 64
    rng = np.random.default_rng(40)
    items = [(L, v) for L in crc_lengths() for v in range(5)]
    frames = []                                            # (dac_rate, sbr, starts, {au index: variant})
    short = [it for it in items if 11 + it[0] + 2 <= 4095]
    i = 0
    while i < len(short):
        starts, var = [11], {}
        while i < len(short) and len(var) < 5 and starts[-1] + short[i][0] + 2 <= 4095:
            var[len(var)] = short[i][1]
            starts.append(starts[-1] + short[i][0] + 2)
            i += 1
        while len(starts) < 6:                              # fewer than five: fillers of one byte
            starts.append(starts[-1] + 3)
        frames.append((1, 0, starts + [size], var))
    for L, v in items:
        if 11 + L + 2 > 4095:
            frames.append((0, 1, [5, size - L - 2, size], {1: v}))
    data, masks = [], []
    for dac, sbr, starts, var in frames:
        d = data_part(rng, s, dac, sbr, starts)
        mask = (1 << (len(starts) - 1)) - 1
        for a, v in var.items():
            b0, b1 = starts[a], starts[a + 1]
            if v:
                at = [b0, b1 - 3, b1 - 2, b1 - 1][v - 1]
                d[at] ^= 1 << int(rng.integers(0, 8))
                mask &= 0 if at < 11 else ~(1 << a)          # (the longest unit starts at byte 8, under the Fire code)
        data.append(d)
        masks.append(mask)
    return encode(data, s), np.array(masks)


BAD_STARTS = [[100, 100, 600], [300, 100, 600], [100, 101, 600], [100, 102, 600], [100, 103, 600], [100, 300, 900],
              [100, 300, 4095], [100, 300, 880], [100, 300, 878], [0, 300, 600], [1, 300, 600], [2, 300, 600],
              [3, 300, 600], [8, 300, 600], [10, 300, 600], [100, 0, 600], [100, 300, 0], [600, 300, 100]]


@functools.lru_cache(maxsize=None)
def header_cases():
    """[(s, sfs)]: all four (dac_rate, sbr) at s from 1 to 64; a valid Fire code over bad starts (equal, decreasing, gaps
    of 0..3, beyond 110 s, 0..2, inside the header); one bit of each header byte 0..10 wrong (RS made to agree); the header
    damaged within RS capacity; all-zero super-frames and an all-zero header."""
    rng = np.random.default_rng(50)
    out = []
    for s in (1, 3, 8, 24, 37, 38, 64):
        sfs = encode([data_part(rng, s, *c) for c in COMBOS for _ in range(2)], s)
        for f in range(1, len(sfs), 2):                     # the second of each pair with 0..2 errors per column
            for j in range(s):
                hit_column(sfs[f], s, j, rng, int(rng.integers(0, 3)))
        out.append((s, sfs))
    s = 8                                                    # four AUs from byte 8; 110 s = 880
    data = [data_part(rng, s, 0, 0, [8] + b + [880]) for b in BAD_STARTS]
    data += [data_part(rng, s, 1, 0, [11, 14, 17, 500, 499, 600, 880]), data_part(rng, s, 1, 0, [11, 20, 881, 882, 883, 884, 880])]
    for b in range(11):                                      # one bit wrong in header byte b, no RS help
        d = data_part(rng, s, *COMBOS[b % 4])
        d[b] ^= 1 << (b % 8)
        data.append(d)
    d = data_part(rng, s, 1, 0)
    d[:11] = 0
    data.append(d)                                           # an all-zero header over a valid rest
    sfs = encode(data, s)
    out.append((s, np.concatenate([sfs, np.zeros((1, 120 * s), np.uint8)])))
    for s in (8, 24, 64):                                    # every header byte damaged, within RS capacity
        sfs = encode([data_part(rng, s, *c) for c in COMBOS], s)
        sfs[:, :11] ^= rng.integers(1, 256, (4, 11), dtype=np.uint8)
        out.append((s, np.concatenate([sfs, np.zeros((1, 120 * s), np.uint8)])))
    s = 1                                                    # 110 s = 110: starts beyond it
    out.append((s, encode([data_part(rng, s, 0, 0, [8] + b + [110]) for b in ([20, 50, 111], [20, 111, 112], [20, 50, 107])], s)))
    return out


def all_cases():
    yield from rs_cases()
    yield from bitrate_cases()
    yield 64, crc_cases()[0]
    yield from header_cases()


_REF = {}


def expected(s, sfs):
    """reference (data, status) of a case batch, computed once per batch (the batches themselves are cached)"""
    hit = _REF.get(id(sfs))
    if hit is None or hit[0] is not sfs:
        hit = _REF[id(sfs)] = (sfs, R.superframes(sfs, s))
    return hit[1]


# ------------------------------------------------------------------------------------------------------------ CPU
def test_reference_superframe_equals_the_oracle_on_every_case():
    n = 0
    for s, sfs in all_cases():
        data, st = expected(s, sfs)
        for f in range(len(sfs)):
            c, ost, oau = O.dabplus_superframe(sfs[f], s)
            got = [int(st[f][k]) for k in ("firecode_ok", "rs_corrected", "rs_uncorrectable", "num_aus", "au_crc_mask")]
            assert got == ost.tolist() and st[f]["au_start"].tolist() == oau.tolist(), (s, f, got, ost, oau)
            assert (data[f] == c[:110 * s]).all() and not st[f]["reserved"].any(), (s, f)
            n += 1
    assert n > 1500


def test_cases_cover_what_they_claim():
    masks = crc_cases()[1]
    _, st = expected(64, crc_cases()[0])
    assert (st["au_crc_mask"] == masks).all() and st["firecode_ok"].sum() == len(masks) - 1 and not st["rs_corrected"].any()
    kinds = {"corrected": 0, "flagged": 0}
    for s, sfs in rs_cases():
        _, st = expected(s, sfs)
        kinds["corrected"] += int(st["rs_corrected"].sum())
        kinds["flagged"] += int(st["rs_uncorrectable"].sum())
    assert kinds["corrected"] > 300 and kinds["flagged"] > 50
    for s, sfs in bitrate_cases():
        _, st = expected(s, sfs)
        assert st[0]["rs_uncorrectable"] == 0 and st[0]["rs_corrected"] >= s and st[0]["firecode_ok"] == 1, s
    hc = header_cases()
    _, st = expected(*hc[7])                                 # the bad-start and broken-header frames at s = 8
    assert st["firecode_ok"][:len(BAD_STARTS) + 2].all() and not st["firecode_ok"][len(BAD_STARTS) + 2:].any()
    for s, sfs in hc[8:11]:
        _, st = expected(s, sfs)
        assert st["firecode_ok"].tolist() == [1, 1, 1, 1, 0], s


def test_builder_cuts_fit_the_header():
    """synth.build_superframe draws AU starts below 4096 (12-bit header fields) and refuses explicit ones that do not fit."""
    from dabgpu import synth
    for br in (304, 512):
        for seed in range(4):
            sf, starts, _ = synth.build_superframe(np.random.default_rng(seed), br, 1, 0)
            assert max(starts[1:-1]) < 4096
            _, st = R.superframe(sf, br // 8)
            assert st["firecode_ok"] == 1 and st["au_start"][:7].tolist() == starts and st["au_crc_mask"] == 63
    with pytest.raises(AssertionError):
        synth.build_superframe(np.random.default_rng(0), 512, 0, 1, cuts=[4096])


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def sctx(built):
    from conftest import make_ctx
    c = make_ctx()
    yield c
    c.close()


def _records(st):
    return np.ascontiguousarray(st).view(np.int32).reshape(len(st), 16)


def assert_matches(out, st, s, sfs, what=""):
    """GPU (out, status) == reference, byte for byte; flagged columns left exactly as received."""
    want, wst = expected(s, sfs)
    assert out.shape == want.shape and len(st) == len(wst)
    bad = np.flatnonzero((out != want).any(axis=1) | (_records(st) != _records(wst)).any(axis=1))
    if bad.size:
        f = int(bad[0])
        raise AssertionError("%s s=%d: %d of %d super-frames differ; first %d: status %s, want %s; bytes differ at %s"
                             % (what, s, bad.size, len(sfs), f, _records(st)[f].tolist(), _records(wst)[f].tolist(),
                                np.flatnonzero(out[f] != want[f])[:12].tolist()))


def run_dev(ctx, sfs, s, stride=None, offset=0, n=None, bitrate=None, check_sentinels=True):
    """_dev call on device buffers: super-frame f at in + offset + f * stride (garbage between), output and status inside
    sentinel bytes -> (out [n][110 s], status [n]) read back, after checking that no sentinel changed."""
    import torch
    import dabgpu
    n = len(sfs) if n is None else n
    stride = 120 * s if stride is None else stride
    rng = np.random.default_rng(stride * 31 + offset)
    buf = rng.integers(0, 256, offset + max(n - 1, 0) * stride + 120 * s + 64, dtype=np.uint8)
    for f in range(n):
        buf[offset + f * stride:offset + f * stride + 120 * s] = sfs[f]
    pad = 256
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.full((2 * pad + n * 110 * s,), 0xA7, dtype=torch.uint8, device="cuda")
    d_st = torch.full((2 * pad + n * 64,), 0x5B, dtype=torch.uint8, device="cuda")
    try:
        ctx.dabplus_superframes_dev(d_in.data_ptr() + offset, stride, n, 8 * s if bitrate is None else bitrate,
                                    d_out.data_ptr() + pad, d_st.data_ptr() + pad)
    except dabgpu.DabGpuError:                               # a refusal leaves both buffers as they were
        ctx.sync()
        assert (d_out.cpu().numpy() == 0xA7).all() and (d_st.cpu().numpy() == 0x5B).all(), "refused call wrote"
        raise
    ctx.sync()
    o, t = d_out.cpu().numpy(), d_st.cpu().numpy()
    if check_sentinels:
        assert (o[:pad] == 0xA7).all() and (o[pad + n * 110 * s:] == 0xA7).all(), "output written outside its rows"
        assert (t[:pad] == 0x5B).all() and (t[pad + n * 64:] == 0x5B).all(), "status written outside its records"
    return o[pad:pad + n * 110 * s].reshape(n, 110 * s), t[pad:pad + n * 64].copy().view(dabgpu.SUPERFRAME_STATUS_DTYPE)


@pytest.mark.gpu
def test_gpu_rs_edges_and_miscorrections(sctx):
    for s, sfs in rs_cases():
        out, st = sctx.dabplus_superframes(sfs, 8 * s)
        assert_matches(out, st, s, sfs, "rs")
        for f in range(len(sfs)):                           # flagged columns: exactly as received
            for j in range(s):
                if R.rs_decode(sfs[f, j::s]) is None:
                    assert (out[f, j::s] == sfs[f, j:110 * s:s]).all(), (s, f, j)


@pytest.mark.gpu
def test_gpu_every_bitrate(sctx):
    for s, sfs in bitrate_cases():
        out, st = run_dev(sctx, sfs, s)
        assert_matches(out, st, s, sfs, "bitrate")


@pytest.mark.gpu
def test_gpu_access_unit_crcs_at_every_length_class(sctx):
    sfs, masks = crc_cases()
    out, st = run_dev(sctx, sfs, 64)
    assert (st["au_crc_mask"] == masks).all()
    assert_matches(out, st, 64, sfs, "crc")


@pytest.mark.gpu
def test_gpu_headers(sctx):
    for s, sfs in header_cases():
        out, st = sctx.dabplus_superframes(sfs, 8 * s)
        assert_matches(out, st, s, sfs, "header")


@pytest.mark.gpu
def test_gpu_dev_strides_offsets_and_counts(sctx):
    """in_stride 120 s, 120 s + 1, 120 s + 15, 240 s at base offsets 0..15, for even and odd s; n = 0, 1, 2, 8, 9, 3000."""
    for s, sfs in rs_cases()[:2]:                            # s = 24 and s = 5
        for stride in (120 * s, 120 * s + 1, 120 * s + 15, 240 * s):
            for offset in range(16):
                out, st = run_dev(sctx, sfs, s, stride, offset)
                assert_matches(out, st, s, sfs, "stride %d offset %d" % (stride, offset))
    s, sfs = rs_cases()[0]
    for n in (0, 1, 2, 8, 9):
        out, st = run_dev(sctx, sfs, s, n=n)
        want, wst = expected(s, sfs)
        assert (out == want[:n]).all() and (_records(st) == _records(wst)[:n]).all(), n
    big = np.tile(sfs, (250, 1))                                # 3000 super-frames
    out, st = run_dev(sctx, big, s, stride=120 * s + 3, offset=5)
    want, wst = expected(s, sfs)
    assert (out == np.tile(want, (250, 1))).all() and (_records(st) == np.tile(_records(wst), (250, 1))).all()


def _host(ctx, rows, s, kind):
    """The host call on pageable arrays, dabgpu.PinnedArray (coherent page-locked) or torch pin_memory() buffers; the output
    and status rows sit between two sentinel rows."""
    import torch
    import dabgpu
    n = rows.shape[0]
    keep = []
    if kind == "pageable":
        src = rows
        o = np.full((n + 2, 110 * s), 0xA7, np.uint8)
        t = np.full((n + 2) * 64, 0x5B, np.uint8).view(dabgpu.SUPERFRAME_STATUS_DTYPE)
    elif kind == "pinned":
        p_in, p_out, p_st = (dabgpu.PinnedArray(rows.shape, np.uint8), dabgpu.PinnedArray((n + 2, 110 * s), np.uint8),
                             dabgpu.PinnedArray(((n + 2) * 64,), np.uint8))
        keep = [p_in, p_out, p_st]
        src, o, t = p_in.array, p_out.array, p_st.array.view(dabgpu.SUPERFRAME_STATUS_DTYPE)
        src[:] = rows
        o[:] = 0xA7
        p_st.array[:] = 0x5B
    else:
        t_in = torch.from_numpy(rows).pin_memory()
        t_out = torch.full(((n + 2) * 110 * s,), 0xA7, dtype=torch.uint8).pin_memory()
        t_st = torch.full(((n + 2) * 64,), 0x5B, dtype=torch.uint8).pin_memory()
        keep = [t_in, t_out, t_st]
        src, o, t = t_in.numpy(), t_out.numpy().reshape(n + 2, 110 * s), t_st.numpy().view(dabgpu.SUPERFRAME_STATUS_DTYPE)
    ctx.dabplus_superframes(src, 8 * s, out=o[1:n + 1], status=t[1:n + 1])
    raw = t.view(np.uint8).reshape(n + 2, 64)
    assert (o[0] == 0xA7).all() and (o[n + 1] == 0xA7).all() and (raw[0] == 0x5B).all() and (raw[n + 1] == 0x5B).all(), kind
    res = o[1:n + 1].copy(), t[1:n + 1].copy()
    for k in keep:
        if hasattr(k, "close"):
            k.close()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("s", [8, 13])
def test_gpu_host_call_on_every_buffer_kind_equals_dev(sctx, s):
    rng = np.random.default_rng(60 + s)
    sfs = encode([data_part(rng, s, *COMBOS[f % 4]) for f in range(9)], s)
    for f in range(9):
        for j in range(s):
            hit_column(sfs[f], s, j, rng, f % 7)
    dev_out, dev_st = run_dev(sctx, sfs, s)
    assert_matches(dev_out, dev_st, s, sfs, "dev")
    for extra in (0, 7):
        rows = np.concatenate([sfs, rng.integers(0, 256, (9, extra), dtype=np.uint8)], axis=1)
        for n in (1, 2, 5, 8, 9):
            for kind in ("pageable", "pinned", "torch"):
                out, st = _host(sctx, np.ascontiguousarray(rows[:n]), s, kind)
                assert (out == dev_out[:n]).all() and (_records(st) == _records(dev_st)[:n]).all(), (kind, n, extra)


@pytest.mark.gpu
def test_gpu_refusals_leave_the_output_alone(sctx):
    import dabgpu
    import torch
    s, sfs = rs_cases()[0]
    for br, n, stride in [(0, 2, None), (4, 2, None), (513, 2, None), (520, 2, None), (8 * s, 2, 120 * s - 1), (8 * s, 3, 1)]:
        with pytest.raises(dabgpu.DabGpuError):
            run_dev(sctx, sfs[:max(n, 1)], s, stride=stride if stride is not None else 120 * s, n=n, bitrate=br)
        # the same through the host call, pageable and page-locked: error, output and status untouched
        buf = np.ascontiguousarray(sfs[:3]).reshape(-1)
        for kind in ("pageable", "pinned"):
            if kind == "pinned":
                keep = [dabgpu.PinnedArray(buf.shape, np.uint8), dabgpu.PinnedArray((n * 110 * s,), np.uint8),
                        dabgpu.PinnedArray((n * 64,), np.uint8)]
                src, o, t = (k.array for k in keep)
                src[:] = buf
            else:
                keep, src, o, t = [], buf, np.empty(n * 110 * s, np.uint8), np.empty(n * 64, np.uint8)
            o[:] = 0xA7
            t[:] = 0x5B
            rc = sctx._lib.dabgpu_dabplus_superframes(sctx._h, src.ctypes.data, stride if stride is not None else 120 * s, n, br,
                                                      o.ctypes.data, t.ctypes.data)
            assert rc != 0 and (o == 0xA7).all() and (t == 0x5B).all(), (br, n, stride, kind, rc)
            for k in keep:
                k.close()
    torch.cuda.synchronize()
