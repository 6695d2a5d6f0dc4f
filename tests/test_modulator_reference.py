"""The device modulator (mod_kernels.hip, dabgpu_mod_api.hip) held to tests/transmit_reference.py, the transmitter written
from the definition without the library, on every protection profile and at the edges of the encoder's loops.

CPU part: the new reference equals modulator_reference (the dabgpu.synth composition) on every case the GPU part uses, its
samples give back its bits and its bits give back the ETI bytes through decoder_reference, and the case list reaches what
it claims to reach (the coverage table is printed).

GPU part, every case in this order so that a failure says what is wrong: (i) demap() of the device samples puts every
carrier within the carrier budget of an eighth-turn point at unit amplitude and every other bin within it of zero, (ii) the
exponent of that point equals spectrum() on every carrier of every symbol (the message names the first wrong bit's symbol
and sub-channel), (iii) every sample is within the sample budget of modulate(), (iv) every prefix is bit-identical to its
symbol's last 504 samples.  The budgets are derived in transmit_reference's docstring; the worst ratios are printed.

All cases run 5 transmission frames (20 CIFs): the smallest run in which coded records 0..4 are seen at every interleaver
delay and CIFs 15..19 are fully populated.  The state test runs 10 frames per stream (calls of 1, 3, 4 and 2)."""
import functools
import os
import re
import zlib

import numpy as np
import pytest

import decoder_reference as D
import eti_reference as E
import ofdm_reference as O
import sync_reference as S
import tii_reference as TII
import transmit_reference as T

N_FRAMES, N_CIF = 5, 20
CEILING = 1e-4                                       # of the frame's peak: what tests/test_modulator.py allows


# ------------------------------------------------------------------------------------------------ the case list
def uep(bitrate, level):
    return {"bitrate": bitrate, "uep": True, "eep_type": 0, "level": level}


def eep(option, level, bitrate):
    return {"bitrate": bitrate, "uep": False, "eep_type": option, "level": level}


def placed(st, ident, start):
    return dict(st, id=ident, start=start)


def all_profiles():
    """Every UEP row, EEP-A levels 1..4 at 8 kbit/s and at one larger rate each (two for level 2, whose 8 kbit/s row is
    the special one), EEP-B levels 1..4 at 32 kbit/s and one at 64."""
    out = [uep(p.bitrate, p.level) for p in T.uep_rows()]
    out += [eep(0, lv, 8) for lv in (1, 2, 3, 4)]
    out += [eep(0, 1, 24), eep(0, 2, 16), eep(0, 2, 40), eep(0, 3, 72), eep(0, 4, 104)]
    out += [eep(1, lv, 32) for lv in (1, 2, 3, 4)] + [eep(1, 2, 64)]
    return out


def fits(sts):
    return (sum(T.profile_of(s).size_cu for s in sts) <= 864 and len(sts) <= 64 and
            E.frame_length([dict(s, id=0, start=0) for s in sts])[1] <= E.FRAME_BYTES)


def ident(k):
    return (5 * k + 3) % 64                          # distinct for k < 64, and not in the frame's order


def packed_ensembles():
    """First fit, largest first, into as few ensembles as hold them.  Ensemble j lays its sub-channels out from CU 0
    (j mod 3 = 0: the free CUs behind them), up to CU 863 (1: in front) or with the free CUs spread between them (2)."""
    bins = []
    for st in sorted(all_profiles(), key=lambda s: -T.profile_of(s).size_cu):
        for b in bins:
            if fits(b + [st]):
                b.append(st)
                break
        else:
            bins.append([st])
    out = []
    for j, b in enumerate(bins):
        b = b[1::2] + b[0::2]                        # (not sorted by size either)
        free = 864 - sum(T.profile_of(s).size_cu for s in b)
        gap = [0] * len(b)
        if j % 3 == 1:
            gap[0] = free
        elif j % 3 == 2:
            gap = [free // (len(b) + 1)] * len(b)
        cu, sts = 0, []
        for k, st in enumerate(b):
            cu += gap[k]
            sts.append(placed(st, ident(k), cu))
            cu += T.profile_of(st).size_cu
        out.append(sorted(sts, key=lambda s: s["id"]))
    return out


def fullest_ensemble():
    """The longest frame that 864 CUs and 64 streams allow.  Per CU a stream adds most to the frame length (its STC word and
    its bytes) as EEP 4-A at 8 kbit/s (7 words in 4 CUs), then EEP 4-B (25 in 15 at 32 kbit/s, 49 in 30 at 64), every UEP
    row less (at most 25 in 16): the search is over the counts of those three.  The CUs run out first, at 5884 bytes --
    no legal ensemble reaches 6144."""
    kinds = [eep(1, 4, 64), eep(1, 4, 32), eep(0, 4, 8)]
    size = [T.profile_of(s).size_cu for s in kinds]
    words = [1 + 2 * E.stl_of(s) for s in kinds]                 # what a stream adds to FL: its STC word and its data
    best = (0, 0, 0, 0)
    for a in range(65):
        for x in range(65 - a):
            for y in range(65 - a - x):
                fl = 25 + a * words[0] + x * words[1] + y * words[2]
                if a * size[0] + x * size[1] + y * size[2] <= 864 and 4 * fl + 16 <= E.FRAME_BYTES and fl > best[0]:
                    best = (fl, a, x, y)
    sts = [kinds[0]] * best[1] + [kinds[1]] * best[2] + [kinds[2]] * best[3]
    cu, out = 0, []
    for k, st in enumerate(sts[::-1]):
        out.append(placed(st, ident(k), cu))
        cu += T.profile_of(st).size_cu
    return out


PACKED = packed_ensembles()
CASES = {"packed%d" % j: sts for j, sts in enumerate(PACKED)}
EDGES = {
    "8k-eep2a": [placed(eep(0, 2, 8), 1, 0)],                     # 24 bytes, the special row
    "80k-eep4a": [placed(eep(0, 4, 80), 2, 7)],                   # 240 bytes: the tail on thread 240's first pass
    "88k-eep1a": [placed(eep(0, 1, 88), 3, 101)],                 # 264 bytes: a second pass, the tail on it
    "176k-eep2a": [placed(eep(0, 2, 176), 4, 333)],               # 528 bytes: the PRBS table wraps
    "256k-eep3a": [placed(eep(0, 3, 256), 5, 672)],               # 768 bytes: the tail on thread 0's fourth pass, ends at CU 864
    "384k-eep1a": [placed(eep(0, 1, 384), 6, 288)],               # 1152 bytes, 576 CUs, the table wraps twice
}
for _p in T.uep_rows():
    if _p.bitrate == 384:
        EDGES["384k-uep%d" % _p.level] = [placed(uep(384, _p.level), 10 + _p.level, 864 - _p.size_cu if _p.level == 1 else _p.level)]
GEOMETRY = {
    "nst0": [],
    "nst64": [placed(eep(0, 4, 8), ident(k), 4 * k + (k // 8) * 11) for k in range(64)],
    "fullest": fullest_ensemble(),
}
MIXED = [placed(uep(32, 5), 7, 0), placed(eep(0, 2, 8), 33, 450), placed(eep(1, 3, 32), 20, 846)]   # L4 = 0; special row; ends at CU 864
CASES.update(EDGES)
CASES.update(GEOMETRY)
CASES["mixed"] = MIXED


def contents(name, seed=0, n_cif=N_CIF):
    rng = np.random.default_rng([zlib.crc32(name.encode()), seed])
    fibs = rng.integers(0, 256, (n_cif, 3, 32), dtype=np.uint8)
    data = {st["id"]: rng.integers(0, 256, (n_cif, st["bitrate"] * 3), dtype=np.uint8) for st in CASES[name]}
    return fibs, data


@functools.lru_cache(maxsize=None)
def reference(name, seed=0, n_cif=N_CIF, refused=()):
    """The case's contents, ETI frames and reference bits: computed once, never modified."""
    fibs, data = contents(name, seed, n_cif)
    eti = T.build_eti(CASES[name], fibs, data)
    bits = T.frame_bits(CASES[name], fibs, data, refused=refused)
    for a in (fibs, eti, bits) + tuple(data.values()):
        a.setflags(write=False)
    return {"streams": CASES[name], "fibs": fibs, "data": data, "eti": eti, "bits": bits}


# ------------------------------------------------------------------------------------------------ the four checks
def bitwise_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check_iq(got, bits, streams, label, tii=None):
    """(i) .. (iv) on got [n][196608] complex64 against the reference of `bits`; -> the worst ratios to the budgets."""
    got = np.asarray(got)
    n = len(bits)
    assert got.shape == (n, T.NB_FRAME_SAMPLES) and got.dtype == np.complex64
    budget = T.carrier_budget()
    # (i) carrier geometry
    X = T.demap(got)
    e_hat, unused = T.nearest_points(X)
    off = np.abs(X[..., O.DATA_BINS] - T.POINTS[e_hat])
    r_carrier = float(max(off.max(), unused.max()) / budget)
    if off.max() > budget:
        f, l, k = np.unravel_index(np.argmax(off), off.shape)
        pytest.fail("%s: frame %d symbol %d carrier %d is %.3e from the nearest eighth-turn point of unit amplitude (budget %.3e)"
                    % (label, f, l, O.CARRIERS[k], off.max(), budget))
    if unused.max() > budget:
        f, l, k = np.unravel_index(np.argmax(unused), unused.shape)
        pytest.fail("%s: frame %d symbol %d bin %d carries %.3e (budget %.3e)" % (label, f, l, T.UNUSED_BINS[k], unused.max(), budget))
    # (ii) bits
    want = T.spectrum(bits)
    if not (e_hat == want).all():
        if not (e_hat[:, 0] == want[:, 0]).all():
            f, k = np.argwhere(e_hat[:, 0] != want[:, 0])[0]
            pytest.fail("%s: frame %d, the phase reference symbol's carrier %d has exponent %d, not %d"
                        % (label, f, O.CARRIERS[k], e_hat[f, 0, k], want[f, 0, k]))
        hard, ok = T.bits_of(e_hat)
        assert ok.all(), "%s: a step between two symbols that no dibit makes" % label
        f, b = np.argwhere(hard != bits)[0]
        pytest.fail("%s: %d wrong bits, the first in %s" % (label, int((hard != bits).sum()), T.locate(streams, int(f), int(b))))
    # (iii) samples
    ref = T.modulate(bits, tii)
    data = slice(T.NB_NULL, None)
    ratio = np.abs(got[:, data] - ref[:, data]) / T.sample_budget(ref[:, data])
    r_sample = float(ratio.max())
    if r_sample > 1.0:
        f, i = np.unravel_index(np.argmax(ratio), ratio.shape)
        pytest.fail("%s: frame %d sample %d is %.2f budgets from the reference" % (label, f, T.NB_NULL + i, r_sample))
    assert float(np.abs(got - ref).max()) <= CEILING * float(np.abs(ref).max())
    r_null = 0.0
    if tii is None:
        assert not got[:, :T.NB_NULL].any(), "%s: the null symbol is not zeros" % label
    else:
        r_null = float(np.abs(got[:, :T.NB_NULL] - ref[:, :T.NB_NULL]).max() / T.tii_sample_budget())
        assert r_null <= 1.0, "%s: the TII symbol is %.2f budgets from the reference" % (label, r_null)
    # (iv) prefix
    sym = got[:, data].reshape(n, T.NB_SYMBOLS, T.NB_SYM)
    assert bitwise_equal(sym[:, :, :T.NB_CP], sym[:, :, T.NB_FFT:]), "%s: a cyclic prefix is not its symbol's end" % label
    print("modulator vs transmit_reference, %s: worst carrier %.3f, worst sample %.3f%s of the budget"
          % (label, r_carrier, r_sample, "" if tii is None else ", worst TII sample %.3f" % r_null))
    return r_carrier, r_sample


# ------------------------------------------------------------------------------------------------ CPU
def test_reference_imports_nothing_of_the_library():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "transmit_reference.py")).read()
    names = re.findall(r"^\s*(?:import|from)\s+([\w.]+)", src, re.M)
    assert sorted(names) == ["decoder_reference", "eti_reference", "numpy", "ofdm_reference", "sync_reference", "tii_reference"]
    assert not re.search(r"__import__|importlib|\bexec\b|\beval\b", src)
    assert not any(n.split(".")[0] in ("dabgpu", "oracle", "modulator_reference") for n in names)


def test_coverage_of_the_case_list():
    """Asserted from the reference's profiles alone."""
    packed = [st for sts in PACKED for st in sts]
    rows = {(st["bitrate"], st["level"]) for st in packed if st["uep"]}
    table = T.uep_rows()
    assert rows == {(p.bitrate, p.level) for p in table} and len(rows) == 64
    eepa = {(st["level"], st["bitrate"]) for st in packed if not st["uep"] and st["eep_type"] == 0}
    eepb = {(st["level"], st["bitrate"]) for st in packed if not st["uep"] and st["eep_type"] == 1}
    for lv in (1, 2, 3, 4):
        assert (lv, 8) in eepa and any(l == lv and br > 8 for l, br in eepa) and any(l == lv for l, _ in eepb)
    assert D.eep_profile(0, 2, 8).blocks == [(5, 13), (1, 12)] and D.eep_profile(0, 2, 16).blocks == [(1, 14), (11, 13)]
    indices = {pi for st in packed for n, pi in T.profile_of(st).blocks if n > 0}
    # every index that ANY profile holds: the 64 rows and the EEP formulas (whose indices do not depend on the bit rate).
    # Index 21 is in no row of the table and in no EEP formula, so no sub-channel the modulator accepts can run it:
    # 23 of the 24 vectors are all the ABI can reach
    exist = {pi for p in table for n, pi in p.blocks if n > 0} | {pi for o, brs in ((0, (8, 16)), (1, (32,))) for lv in (1, 2, 3, 4)
                                                                  for br in brs for n, pi in D.eep_profile(o, lv, br).blocks}
    assert indices == exist == set(range(1, 25)) - {21}
    l4_zero = [i for i, p in enumerate(table) if p.blocks[3][0] == 0]
    padded = [i for i, p in enumerate(table) if p.padding]
    assert l4_zero and padded and 4 in padded
    starts_at_0 = ends_at_864 = with_gaps = 0
    print("\nensemble  streams  CUs  ETI bytes  puncturing indices")
    for name, sts in CASES.items():
        used = np.zeros(864, int)
        for st in sts:
            used[st["start"]:st["start"] + T.profile_of(st).size_cu] += 1
        assert used.max(initial=0) <= 1 and len(sts) <= 64 and len({st["id"] for st in sts}) == len(sts)
        assert all(st["start"] + T.profile_of(st).size_cu <= 864 for st in sts)
        length = E.frame_length(sts)[1]
        assert length <= E.FRAME_BYTES
        if name.startswith("packed"):
            order = sorted(sts, key=lambda s: s["start"])
            starts_at_0 += order[0]["start"] == 0
            ends_at_864 += order[-1]["start"] + T.profile_of(order[-1]).size_cu == 864
            with_gaps += int(used.sum()) < 864 and any(used[a] == 0 and used[a:].any() for a in range(864))
        print("%-11s %5d  %4d  %5d   %s" % (name, len(sts), used.sum(), length,
                                            sorted({pi for st in sts for n, pi in T.profile_of(st).blocks if n > 0})))
    print("UEP rows 64 of 64 (L4 = 0: %s; padding: %s); EEP-A %s; EEP-B %s; indices %s; %d packed ensembles"
          % (l4_zero, padded, sorted(eepa), sorted(eepb), sorted(indices), len(PACKED)))
    assert starts_at_0 >= 1 and ends_at_864 >= 1 and with_gaps >= 1 and len(PACKED) <= 12
    assert len(GEOMETRY["nst64"]) == 64 and E.frame_length(GEOMETRY["fullest"])[1] == 5884
    # the byte-loop edges: bytes per codeword
    assert [CASES[n][0]["bitrate"] * 3 for n in ("8k-eep2a", "80k-eep4a", "88k-eep1a", "176k-eep2a", "256k-eep3a", "384k-eep1a")] == \
        [24, 240, 264, 528, 768, 1152]
    assert T.profile_of(CASES["384k-eep1a"][0]).size_cu == 576 and sum(n.startswith("384k-uep") for n in CASES) >= 2


def synth_modulate64(bits, tii=None):
    """dabgpu.synth.modulate_frame without its cast to complex64: the same tables, the same running product z_l = z_(l-1) y."""
    from dabgpu import synth
    car, prs = synth.carrier_of_data_index(), synth.prs_carriers()
    out = np.zeros((len(bits), synth.NB_FRAME_SAMPLES), np.complex128)
    scale = synth.NB_FFT / np.sqrt(synth.NB_CARRIERS)
    k = np.arange(-768, 769)
    for f, fb in enumerate(np.asarray(bits, np.uint8).reshape(-1, 75, synth.NB_SYM_BITS)):
        if tii is not None:
            out[f, :synth.NB_NULL] = synth.tii_null([tii])       # (complex64: the TII symbol is compared at that precision)
        z = prs.copy()
        pos = synth.NB_NULL
        for l in range(synth.NB_SYMBOLS):
            if l > 0:
                p = fb[l - 1].astype(np.float64)
                q = ((1 - 2 * p[:synth.NB_CARRIERS]) + 1j * (1 - 2 * p[synth.NB_CARRIERS:])) / np.sqrt(2.0)
                y = np.ones(2 * 768 + 1, np.complex128)
                y[car + 768] = q
                z = z * y
            spec = np.zeros(synth.NB_FFT, np.complex128)
            spec[k % synth.NB_FFT] = z
            spec[0] = 0
            t = np.fft.ifft(spec) * scale
            out[f, pos:pos + synth.NB_CP] = t[-synth.NB_CP:]
            out[f, pos + synth.NB_CP:pos + synth.NB_SYM] = t
            pos += synth.NB_SYM
    return out


# float64 rounding between the two restatements: synth multiplies 75 unit factors into every carrier (a complex product
# is 4 roundings), this reference looks the point up; 1536 carriers of 1 / sqrt(1536) each add up in a sample, and the
# two inverse transforms round 64 times the peak at the very most
def float64_bound(peak):
    return 75 * 4 * 2.0 ** -53 * 1536 / np.sqrt(1536) + 64 * 2.0 ** -53 * peak


@pytest.mark.parametrize("name", list(CASES))
def test_reference_equals_the_synth_composition_and_decodes(name):
    import modulator_reference as M
    ref = reference(name)
    sts, bits = ref["streams"], ref["bits"]
    # frame bits: exact
    theirs = M.frame_bits(sts, ref["fibs"], ref["data"])
    assert theirs.shape == bits.shape and (theirs == bits).all(), name
    # samples: float64 rounding
    mine = T.modulate(bits)
    peak = float(np.abs(mine).max())
    theirs = synth_modulate64(bits)
    assert float(np.abs(mine - theirs).max()) <= float64_bound(peak), name
    # the derived budget lies under the old ceiling
    assert float(T.sample_budget(mine).max()) <= CEILING * peak / 10 and T.tii_sample_budget() <= CEILING * peak / 10
    # samples -> carriers -> differential decision -> the bits
    e_hat, unused = T.nearest_points(T.demap(mine))
    assert (e_hat == T.spectrum(bits)).all() and unused.max() < 1e-12
    hard, ok = T.bits_of(e_hat)
    assert ok.all() and (hard == bits).all()
    # the checks of the GPU part pass the reference's own samples rounded to float32 (half an ulp, far inside the budget)
    if name in ("mixed", "nst0"):
        r = check_iq(mine.astype(np.complex64), bits, sts, name + " (the reference in float32)")
        assert max(r) < 0.1
    # bits -> de-interleaver -> Viterbi -> the ETI bytes, for the logical frames whose 16 CIFs are all there
    fic = D.fic_reference(2 * hard[:, :T.NB_FIC_BITS].astype(np.int64) - 1)
    assert (fic.fib.reshape(N_CIF, 3, 32) == ref["fibs"]).all()
    cifs = 2 * hard[:, T.NB_FIC_BITS:].reshape(N_CIF, T.NB_CIF_BITS).astype(np.int64) - 1
    for st in sts:
        p = T.profile_of(st)
        a = 64 * st["start"]
        lf, _ = D.time_deinterleave(cifs[:, a:a + 64 * p.size_cu])
        dec = D.viterbi(D.depuncture(lf[15:, :p.kept], p.mask), stats=False)
        out = np.packbits(dec.bits() ^ D.prbs(p.nsteps - 6)[None, :], axis=1)
        assert (out == ref["data"][st["id"]][:N_CIF - 15]).all(), (name, st)


def test_reference_with_tii_gain_history_and_refusals():
    import modulator_reference as M
    from dabgpu import synth
    ref = reference("mixed")
    sts, bits = ref["streams"], ref["bits"]
    for main, sub in ((0, 0), (69, 23), (37, 11)):
        mine = T.modulate(bits[:1], tii=(main, sub), gain=-2.0)
        theirs = synth_modulate64(bits[:1], tii=(sub, main)) * -2.0
        assert np.abs(mine - theirs).max() <= 2 * 2.0 ** -24 * np.abs(theirs[:, :T.NB_NULL]).max()       # (synth's null is complex64)
        assert np.abs(mine[:, T.NB_NULL:] - theirs[:, T.NB_NULL:]).max() <= 2 * float64_bound(np.abs(mine).max())
        N = T.demap_null(mine / -2.0)[0]
        on = np.array(TII.transmitter_carriers(sub, main)) % T.NB_FFT
        assert len(on) == 32 and np.abs(N[on] - S.R[on]).max() < 1e-12 and np.abs(np.delete(N, on)).max() < 1e-12
    assert (M.modulate(bits[:2]) == synth_modulate64(bits[:2]).astype(np.complex64)).all()   # the float64 copy IS synth's arithmetic
    assert max(check_iq(T.modulate(bits[:2], tii=(37, 11)).astype(np.complex64), bits[:2], sts, "the reference in float32, TII", tii=(37, 11))) < 0.1
    # refused frames are zero bytes
    fibs, data = contents("mixed")
    theirs = M.frame_bits(sts, fibs, data, refused=(6, 13))
    assert (T.frame_bits(sts, fibs, data, refused=(6, 13)) == theirs).all() and not (theirs == bits).all()
    # two calls with the history carried are one call
    first, hist = T.frame_bits(sts, fibs[:8], {i: d[:8] for i, d in data.items()}, return_history=True)
    second = T.frame_bits(sts, fibs[8:], {i: d[8:] for i, d in data.items()}, history=hist)
    assert (np.concatenate([first, second]) == bits).all()
    assert T.status(8, refused=(6,)) == [(0, 0), (1, 4)] and T.status(8, count0=2) == [(2, 0), (2, 0)]


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def mctx(built):
    from conftest import make_ctx
    c = make_ctx(None, max_frames=64)
    yield c
    c.close()


def library_streams(sts):
    import dabgpu
    return [(st["id"], dabgpu.uep_subchannel(T.uep_index(st["bitrate"], st["level"]), st["start"]) if st["uep"] else
             dabgpu.subchannel(st["start"], st["bitrate"], level=st["level"], eep_type=st["eep_type"])) for st in sts]


def run_mod(ctx, sts, eti, **kw):
    """eti: numpy [n_cif][6144] or [n_streams][n_cif][6144] -> (iq tensor [n_frames][196608], status records, state tensor)."""
    import dabgpu
    import torch
    e = np.asarray(eti)
    d = torch.from_numpy(np.array(e if e.ndim == 3 else e[None])).cuda()           # (a writable copy)
    iq, st, state = ctx.modulate_eti(d, library_streams(sts), **kw)
    return iq, st.cpu().numpy().view(dabgpu.MOD_STATUS_DTYPE).reshape(-1), state


def clean(st, n):
    return len(st) == n and not st["flags"].any() and not st["refused"].any() and not st["reserved"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_every_case(mctx, name):
    """The packed ensembles (every profile), the byte-loop edges, nst = 0 and 64, the fullest frame: one plan, one call."""
    ref = reference(name)
    iq, st, _ = run_mod(mctx, ref["streams"], ref["eti"])
    assert clean(st, N_FRAMES)
    check_iq(iq.cpu().numpy(), ref["bits"], ref["streams"], name)
    if name == "nst0":
        assert not ref["bits"][:, T.NB_FIC_BITS:].any()         # the MSC carriers carry the all-zero bits


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["packed0", "packed%d" % (len(PACKED) - 1)])
def test_gpu_packed_batch_of_two(mctx, name):
    import torch
    a, b = reference(name), reference(name, seed=1)
    assert not (a["bits"] == b["bits"]).all()
    iq, st, _ = run_mod(mctx, a["streams"], np.stack([a["eti"], b["eti"]]))
    alone, _, _ = run_mod(mctx, a["streams"], a["eti"])
    assert clean(st, 2 * N_FRAMES) and torch.equal(iq[:N_FRAMES], alone)
    check_iq(iq[N_FRAMES:].cpu().numpy(), b["bits"], b["streams"], name + ", stream 1 of a batch of two")


@pytest.mark.gpu
def test_gpu_state_across_a_batch(mctx):
    """Three streams in calls of 1, 3, 4 and 2 frames with the state carried, two of them changing places between the calls
    together with their state records: bit-identical to one call of 10 frames per stream, which equals the reference."""
    import torch
    n_cif = 40
    refs = [reference("mixed", seed=s, n_cif=n_cif) for s in (10, 11, 12)]
    etis = np.stack([r["eti"] for r in refs])
    one, st, _ = run_mod(mctx, MIXED, etis)
    assert clean(st, 30)
    one = one.reshape(3, 10, -1)
    for s in range(3):
        check_iq(one[s].cpu().numpy(), refs[s]["bits"], MIXED, "10 frames in one call, stream %d" % s)
    state = {s: None for s in range(3)}
    parts = {s: [] for s in range(3)}
    f0 = 0
    for frames, order in ((1, (0, 1, 2)), (3, (2, 1, 0)), (4, (2, 0, 1)), (2, (0, 2, 1))):
        sin = None if f0 == 0 else torch.stack([state[s] for s in order])
        iq, st, sout = run_mod(mctx, MIXED, etis[list(order), 4 * f0:4 * (f0 + frames)], state=sin)
        assert clean(st, 3 * frames)
        for pos, s in enumerate(order):
            parts[s].append(iq[pos * frames:(pos + 1) * frames])
            state[s] = sout[pos].clone()
        f0 += frames
    for s in range(3):
        assert torch.equal(torch.cat(parts[s]), one[s]), "stream %d" % s
    assert not torch.equal(state[0], state[1]) and not torch.equal(state[1], state[2])


@pytest.mark.gpu
def test_gpu_refused_frame_in_one_stream(mctx):
    import torch
    refs = [reference("mixed", seed=s) for s in (20, 21, 22)]
    etis = np.stack([r["eti"] for r in refs])
    good, st, _ = run_mod(mctx, MIXED, etis)
    assert clean(st, 15)
    etis[1, 9, 1] ^= 0x10                                        # FSYNC of ETI frame 9 of stream 1
    iq, st, _ = run_mod(mctx, MIXED, etis)
    want = [(0, 0)] * 5 + T.status(N_CIF, refused=(9,)) + [(0, 0)] * 5
    assert [(int(x["flags"]), int(x["refused"])) for x in st] == want and want[7] == (T.BAD_INPUT, 2) and not st["reserved"].any()
    iq, good = iq.reshape(3, N_FRAMES, -1), good.reshape(3, N_FRAMES, -1)
    assert torch.equal(iq[0], good[0]) and torch.equal(iq[2], good[2]) and not torch.equal(iq[1], good[1])
    zeroed = reference("mixed", seed=21, refused=(9,))
    assert not (zeroed["bits"] == refs[1]["bits"]).all()
    check_iq(iq[1].cpu().numpy(), zeroed["bits"], MIXED, "ETI frame 9 refused")


@pytest.mark.gpu
@pytest.mark.parametrize("main,sub", [(0, 0), (69, 23), (37, 11)])
def test_gpu_tii_null_symbol(mctx, main, sub):
    import dabgpu
    import torch
    ref = reference("mixed")
    plain, _, _ = run_mod(mctx, MIXED, ref["eti"])
    iq, st, _ = run_mod(mctx, MIXED, ref["eti"], cfg=dabgpu.mod_cfg(tii_main=main, tii_sub=sub))
    assert clean(st, N_FRAMES) and torch.equal(iq[:, T.NB_NULL:], plain[:, T.NB_NULL:])
    got = iq.cpu().numpy()
    check_iq(got, ref["bits"], MIXED, "TII (%d, %d)" % (main, sub), tii=(main, sub))
    # carrier by carrier: the transmitter's 32 carriers carry the PRS phase at a data carrier's amplitude, every other bin nothing
    N = T.demap_null(got[:, :T.NB_NULL])
    on = np.array(TII.transmitter_carriers(sub, main)) % T.NB_FFT
    off = np.setdiff1d(np.arange(T.NB_FFT), on)
    worst = max(float(np.abs(N[:, on] - S.R[on][None, :]).max()), float(np.abs(N[:, off]).max())) / T.tii_carrier_budget()
    print("modulator vs transmit_reference, TII (%d, %d): worst carrier of the null symbol %.3f of the budget" % (main, sub, worst))
    assert len(on) == 32 and worst <= 1.0
    # the cyclic extension over the 2656 samples: the first 608 are the last 608
    assert bitwise_equal(got[:, :T.NB_NULL - T.NB_FFT], got[:, T.NB_FFT:T.NB_NULL])
    assert bitwise_equal(got[0, :T.NB_NULL], got[4, :T.NB_NULL])


@pytest.mark.gpu
def test_gpu_gain_is_an_exact_scaling(mctx):
    import dabgpu
    import torch
    ref = reference("mixed")
    unit, _, _ = run_mod(mctx, MIXED, ref["eti"], cfg=dabgpu.mod_cfg(tii_main=5, tii_sub=6))
    assert bool(unit[:, :T.NB_NULL].any())
    for gain in (0.5, -2.0):
        iq, st, _ = run_mod(mctx, MIXED, ref["eti"], cfg=dabgpu.mod_cfg(gain=gain, tii_main=5, tii_sub=6))
        assert clean(st, N_FRAMES) and torch.equal(torch.view_as_real(iq), torch.view_as_real(unit) * gain), gain
