"""dabgpu_decode_ensembles_dev: a batch of ensembles that each have their own multiplex, decoded in one call.  Every
expected value comes from the transmitted bytes of the multiplexes (tests/ensembles_reference.py, dabgpu.synth), from the
oracle, or from the per-stream dabgpu_decode_frames_dev (one call per stream, n_streams = 1) -- never from the call under
test; every comparison is byte-exact."""
import numpy as np
import pytest
import torch

import dabgpu
from dabgpu import synth
from conftest import make_ctx

import ensembles_reference as E

pytestmark = pytest.mark.gpu

ARG, PROFILE = -1, -5
FB = dabgpu.NB_FRAME_BITS

# four streams that differ in every respect (the numbers: capacity units)
S0 = [("eep", 0, 3, 64, 0), ("uep", 4, 48), ("eep", 1, 2, 32, 100)]        # 64 kbit/s EEP 3-A at CU 0, a UEP row with padding, EEP 2-B
S1 = []                                                                     # FIC only
S2 = [("eep", 0, 2, 32, 0), ("uep", 15, 40)]                                # CU 0 again: another profile, another size
S3 = [("eep", 0, 3, 1152, 0)]                                               # 27 654 steps: no [64][words] tile of that fits into LDS
# more entries than a by-value pack of 16 holds, in ONE stream: 20 x 8 kbit/s EEP 2-A of 8 CU
MANY = [("eep", 0, 2, 8, 8 * i) for i in range(20)]
ONE = [("eep", 0, 4, 16, 300)]
FIVE = [("eep", 0, 3, 8, 0), ("uep", 0, 6), ("eep", 1, 4, 32, 22), ("eep", 0, 1, 8, 37), ("eep", 0, 2, 16, 49)]


def dev():
    return torch.device("cuda", 0)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Batch:
    """n_streams x fps frames of the given multiplexes as soft bits, with a carried history for every sub-channel but the
    first of each stream (that one starts from erasures)."""

    def __init__(self, plexes, fps, noise_seed=None, first=0):
        self.plexes, self.fps, self.n_streams = plexes, fps, len(plexes)
        rng = None if noise_seed is None else np.random.default_rng(noise_seed)
        self.soft = np.concatenate([m.soft(fps, first, rng) for m in plexes])
        self.hist = []
        for m in plexes:
            before = m.soft(4, first - 4, rng)
            self.hist.append([None if k == 0 else np.ascontiguousarray(E.cif_rows(before, sc)[-15:]) for k, sc in enumerate(m.scs)])
        self.scs = [m.scs for m in plexes]

    def stream_soft(self, s):
        return self.soft[s * self.fps:(s + 1) * self.fps]


class Result:
    def __init__(self, fib, ok, outs, houts):
        self.fib, self.ok, self.outs, self.houts = fib, ok, outs, houts


def buffers(batch, fps, misalign=0, fill=0):
    n = batch.n_streams * fps
    fib = torch.full((n, 12, 32), fill, dtype=torch.uint8, device=dev())
    ok = torch.full((n, 12), fill, dtype=torch.uint8, device=dev())
    outs = [[torch.full((misalign + fps * 4 * sc.bitrate_kbps * 3,), fill, dtype=torch.uint8, device=dev()) for sc in lst] for lst in batch.scs]
    houts = [[torch.full((15, sc.length * 64), fill - 256 if fill > 127 else fill, dtype=torch.int8, device=dev()) for sc in lst] for lst in batch.scs]
    return fib, ok, outs, houts


def collect(batch, fps, fib, ok, outs, houts, misalign=0):
    return Result(fib.cpu().numpy(), ok.cpu().numpy(),
                  [[o[misalign:].cpu().numpy().reshape(fps * 4, -1) for o in lst] for lst in outs],
                  [[h.cpu().numpy() for h in lst] for lst in houts])


def ragged(c, batch, soft_t, hin_t, misalign=0, with_fic=True):
    fps = batch.fps
    fib, ok, outs, houts = buffers(batch, fps, misalign)
    c.decode_ensembles_dev(soft_t.data_ptr(), FB, batch.n_streams, fps, fib.data_ptr() if with_fic else None,
                           ok.data_ptr() if with_fic else None, batch.scs,
                           [[None if h is None else h.data_ptr() for h in lst] for lst in hin_t],
                           [[h.data_ptr() for h in lst] for lst in houts], [[o.data_ptr() + misalign for o in lst] for lst in outs], None)
    c.sync()
    return collect(batch, fps, fib, ok, outs, houts, misalign)


def per_stream(c, batch, soft_t, hin_t):
    """the reference a caller has without the new entry point: one dabgpu_decode_frames_dev per stream"""
    fps = batch.fps
    fib, ok, outs, houts = buffers(batch, fps)
    for s in range(batch.n_streams):
        c.decode_frames_dev(soft_t.data_ptr() + s * fps * FB, FB, 1, fps, fib.data_ptr() + s * fps * 12 * 32, ok.data_ptr() + s * fps * 12,
                            batch.scs[s], [None if h is None else h.data_ptr() for h in hin_t[s]], [h.data_ptr() for h in houts[s]],
                            [o.data_ptr() for o in outs[s]], None)
    c.sync()
    return collect(batch, fps, fib, ok, outs, houts)


def hist_to_dev(batch):
    return [[None if h is None else to_dev(h) for h in lst] for lst in batch.hist]


def assert_same(a, b, what):
    assert (a.fib == b.fib).all() and (a.ok == b.ok).all(), what
    for s, (la, lb) in enumerate(zip(a.outs, b.outs)):
        assert len(la) == len(lb)
        for k in range(len(la)):
            assert (la[k] == lb[k]).all(), (what, "out", s, k)
            assert (a.houts[s][k] == b.houts[s][k]).all(), (what, "history", s, k)


def assert_oracle(batch, got):
    """Every soft bit of these batches keeps the transmitted sign, so equal bytes cannot show a lost or misplaced soft bit;
    test_decoder_profiles.py runs the by-table launch on inputs that can."""
    ofib, ook = E.oracle_fic(batch.soft)
    assert (got.fib == ofib).all() and (got.ok == ook).all()
    for s, m in enumerate(batch.plexes):
        for k, spec in enumerate(m.specs):
            out, hist = E.oracle_subchannel(batch.stream_soft(s), spec, batch.hist[s][k])
            assert (got.outs[s][k] == out).all(), (s, k)
            assert (got.houts[s][k] == hist).all(), (s, k)


def assert_sent(batch, got, first=0):
    """a noise-free batch: every FIB as sent, every sub-channel's bytes as sent 15 CIFs earlier (from CIF 15 on where the
    sub-channel started from erasures)"""
    for s, m in enumerate(batch.plexes):
        want = m.fibs[(first + np.arange(batch.fps)) % m.n_cycle]
        assert (got.fib[s * batch.fps:(s + 1) * batch.fps] == want).all() and got.ok.all()
        for k in range(len(m.specs)):
            for t in range(0 if batch.hist[s][k] is not None else 15, 4 * batch.fps):
                assert (got.outs[s][k][t] == m.sent(k, t, first)).all(), (s, k, t)


def took_the_grouped_launch(c):
    """while timing is on, a grouped lane decode -- and nothing else -- leaves the parts of its one timed slot behind"""
    whole, n = c.mean_kernel_ms(2)
    try:
        _, n_parts = c.mean_kernel_ms(4)
    except dabgpu.DabGpuError:
        return False
    return n == 1 and n_parts == 1


@pytest.fixture(scope="module")
def plexes(built):
    return {name: E.Multiplex(seed, specs) for name, seed, specs in
            (("S0", 1, S0), ("S1", 2, S1), ("S2", 3, S2), ("S3", 4, S3), ("MANY", 5, MANY), ("ONE", 6, ONE), ("FIVE", 7, FIVE))}


@pytest.fixture(scope="module")
def ref_ctx(built):
    c = make_ctx(None, max_frames=64)
    yield c
    c.close()


@pytest.fixture()
def timed_ctx(built):
    c = make_ctx(None, max_frames=64)
    c.set_timing(True)
    yield c
    c.close()


@pytest.mark.parametrize("names", [("S0", "S1", "S2", "S3"), ("MANY", "ONE", "FIVE")], ids=["different_plans", "more_entries_than_a_pack"])
def test_one_call_decodes_every_ensembles_own_plan(plexes, ref_ctx, timed_ctx, names):
    """16 frames a stream: exactly one 64-codeword group per entry.  different_plans: three sub-channels / none / two, one
    of them at another stream's start address / one too long for the traceback's LDS tile.  more_entries_than_a_pack: 20
    sub-channels in one stream (a by-value pack holds 16), 1 and 5 in the others."""
    ms = [plexes[n] for n in names]
    noisy = Batch(ms, 16, noise_seed=11)
    soft_t, hin_t = to_dev(noisy.soft), hist_to_dev(noisy)
    got = ragged(timed_ctx, noisy, soft_t, hin_t)
    assert took_the_grouped_launch(timed_ctx)
    assert_same(got, per_stream(ref_ctx, noisy, soft_t, hin_t), "per-stream calls")
    assert_oracle(noisy, got)
    clean = Batch(ms, 16)
    got = ragged(timed_ctx, clean, to_dev(clean.soft), hist_to_dev(clean))
    assert_sent(clean, got)
    # sub-channels only (no FIC): the same bytes, FIBs untouched
    only = ragged(timed_ctx, clean, to_dev(clean.soft), hist_to_dev(clean), with_fic=False)
    assert not only.fib.any() and not only.ok.any()
    only.fib, only.ok = got.fib, got.ok
    assert_same(only, got, "without the FIC")


def test_two_calls_continue_as_one(plexes, ref_ctx, timed_ctx):
    """history_out of 16 frames is history_in of the next 16: together the bytes of one call of 32 frames (two groups per
    entry) and of the per-stream reference"""
    ms = [plexes["S0"], plexes["S2"], plexes["S1"]]
    whole = Batch(ms, 32, noise_seed=21)
    soft_t, hin_t = to_dev(whole.soft), hist_to_dev(whole)
    one = ragged(timed_ctx, whole, soft_t, hin_t)
    assert took_the_grouped_launch(timed_ctx)
    assert_same(one, per_stream(ref_ctx, whole, soft_t, hin_t), "per-stream calls")
    halves = []
    for h in (0, 1):
        part = Batch(ms, 16)
        part.soft = np.concatenate([whole.stream_soft(s)[16 * h:16 * h + 16] for s in range(3)])
        part.hist = whole.hist if h == 0 else halves[0].houts
        halves.append(ragged(timed_ctx, part, to_dev(part.soft), hist_to_dev(part)))
    for s in range(3):
        f = slice(32 * s, 32 * s + 32)
        assert (np.concatenate([halves[0].fib[16 * s:16 * s + 16], halves[1].fib[16 * s:16 * s + 16]]) == one.fib[f]).all()
        assert (np.concatenate([halves[0].ok[16 * s:16 * s + 16], halves[1].ok[16 * s:16 * s + 16]]) == one.ok[f]).all()
        for k in range(len(ms[s].specs)):
            assert (np.concatenate([halves[0].outs[s][k], halves[1].outs[s][k]]) == one.outs[s][k]).all(), (s, k)
            assert (halves[1].houts[s][k] == one.houts[s][k]).all(), (s, k)
    assert_oracle(whole, one)


@pytest.mark.parametrize("fps,misalign", [(3, 1), (3, 0), (16, 1)])
def test_shapes_that_do_not_qualify_give_the_same_bytes(plexes, ref_ctx, timed_ctx, fps, misalign):
    """streams that are no whole 64-codeword groups, outputs off the 4-byte grid: part by part, stream by stream"""
    ms = [plexes["S0"], plexes["S1"], plexes["S2"]]
    noisy = Batch(ms, fps, noise_seed=31)
    soft_t, hin_t = to_dev(noisy.soft), hist_to_dev(noisy)
    got = ragged(timed_ctx, noisy, soft_t, hin_t, misalign=misalign)
    assert not took_the_grouped_launch(timed_ctx)
    assert_same(got, per_stream(ref_ctx, noisy, soft_t, hin_t), "per-stream calls")
    assert_oracle(noisy, got)


def test_refusals_leave_every_output_as_it_was(plexes, ref_ctx, timed_ctx):
    ms = [plexes["S0"], plexes["S2"]]
    batch = Batch(ms, 16, noise_seed=41)
    soft_t, hin_t = to_dev(batch.soft), hist_to_dev(batch)
    want = per_stream(ref_ctx, batch, soft_t, hin_t)
    c = timed_ctx
    sc = dabgpu.subchannel

    def refused(status, scs, d_out=None, sc_first=None):
        fib, ok, outs, _ = buffers(batch, 16, fill=0xA5)
        pool = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device=dev())     # where the entries of a bad plan point
        if d_out is None:
            d_out = [[pool.data_ptr()] * len(lst) for lst in scs]
        none = [[None] * len(lst) for lst in scs]
        with pytest.raises(dabgpu.DabGpuError) as e:
            c.decode_ensembles_dev(soft_t.data_ptr(), FB, 2, 16, fib.data_ptr(), ok.data_ptr(), scs, none, none, d_out, None,
                                   sc_first=sc_first)
        assert e.value.status == status
        c.sync()
        assert (fib == 0xA5).all() and (ok == 0xA5).all() and (pool == 0xA5).all()
        assert all((o == 0xA5).all() for lst in outs for o in lst)
        # ... and the next valid call is right
        assert_same(ragged(c, batch, soft_t, hin_t), want, "after a refusal")
        return outs

    good = batch.scs
    # two entries overlap inside ONE stream
    refused(ARG, [good[0] + [sc(40, 8, level=3)], good[1]])
    # sc_first decreases / does not start at 0
    refused(ARG, good, sc_first=[0, 4, 3])
    refused(ARG, good, sc_first=[1, 3, 5])
    # more than 64 entries in a stream (65 x 8 kbit/s EEP 4-A, 4 CU each: nothing else is wrong with them)
    refused(ARG, [[sc(4 * i, 8, level=4) for i in range(65)], good[1]])
    # an entry without an output
    mine = buffers(batch, 16, fill=0xA5)[2]
    d_out = [[o.data_ptr() for o in lst] for lst in mine]
    d_out[1][1] = None
    refused(ARG, good, d_out=d_out)
    assert all((o == 0xA5).all() for lst in mine for o in lst)
    # a descriptor that names no profile (47 CU is no EEP 3-A size)
    refused(PROFILE, [good[0], [dabgpu.Subchannel(0, 47, 0, 0, 3, 64)]])
    # the same capacity units in two DIFFERENT streams are two ensembles' own business (S0 and S2 both start at CU 0)
    assert good[0][0].start_address == good[1][0].start_address == 0
    assert_same(ragged(c, batch, soft_t, hin_t), want, "shared capacity units")


# (services, dab_services) of dabgpu.synth.ServiceEnsemble: three multiplexes that announce themselves in their FIC
ORGANISATIONS = [
    ([("Alpha", 0xC001, 1, 0, 3, 64, 100), ("Beta", 0xC002, 2, 1, 2, 32, 0)], [("Gamma", 0xC003, 3, 17, 30)]),
    ([("Delta", 0xC101, 9, 0, 1, 8, 700), ("Eps", 0xC102, 4, 0, 4, 48, 40), ("Zeta", 0xC103, 7, 1, 4, 64, 300),
      ("Eta", 0xC104, 5, 0, 2, 8, 0)], []),
    ([], [("Theta", 0xC201, 11, 0, 500), ("Iota", 0xC202, 12, 33, 20)]),
]


def test_unknown_ensembles_end_to_end(built, timed_ctx):
    """IQ of three different multiplexes -> front end -> FIC pass (a ragged call without entries) -> dabgpu_fig_subchannels
    per stream -> one ragged call with those plans: every sub-channel's bytes are what was transmitted"""
    fps, L = 16, 76 * 2552
    ens = [synth.ServiceEnsemble(seed=60 + k, services=sv, dab_services=dab, n_frames=5, extras=False)
           for k, (sv, dab) in enumerate(ORGANISATIONS)]
    rng = np.random.default_rng(3)
    iq = []
    for e in ens:
        tx = e.iq()[np.arange(fps) % 5]                              # the cyclic multiplex, 16 frames of it
        rx = synth.channel(tx.ravel(), snr_db=20.0, rng=rng).reshape(fps, -1)
        iq.append(rx[:, synth.NB_NULL:synth.NB_NULL + L])
    d_iq = to_dev(np.concatenate(iq).astype(np.complex64))
    d_soft = torch.zeros((3 * fps, FB), dtype=torch.int8, device=dev())
    c = timed_ctx
    c.streams_reset(3)
    c.ofdm_demod_streams_dev(d_iq.data_ptr(), L, 3, fps, 0.9, d_soft.data_ptr(), None, None)
    fib = torch.zeros((3 * fps, 12, 32), dtype=torch.uint8, device=dev())
    ok = torch.zeros((3 * fps, 12), dtype=torch.uint8, device=dev())
    c.decode_ensembles_dev(d_soft.data_ptr(), FB, 3, fps, fib.data_ptr(), ok.data_ptr(), [[], [], []], None, None, None, None)
    c.sync()
    fib_h, ok_h = fib.cpu().numpy(), ok.cpu().numpy()
    assert ok_h.all()
    plans = [dabgpu.fig_subchannels(fib_h[s * fps:(s + 1) * fps], ok_h[s * fps:(s + 1) * fps]) for s in range(3)]
    assert [len(p) for p in plans] == [3, 4, 2]
    outs = [[torch.zeros((fps * 4, sc.bitrate_kbps * 3), dtype=torch.uint8, device=dev()) for sc in p] for p in plans]
    c.decode_ensembles_dev(d_soft.data_ptr(), FB, 3, fps, fib.data_ptr(), ok.data_ptr(), plans, None, None,
                           [[o.data_ptr() for o in lst] for lst in outs], None)
    c.sync()
    for s, e in enumerate(ens):
        assert (fib.cpu().numpy()[s * fps:(s + 1) * fps] == e.fibs[np.arange(fps) % 5]).all()
        sent = {start: data for (*_r, start), data in zip(e.services, e.msc_bytes)}
        sent.update({start: data for (*_r, start), data in zip(e.dab_services, e.mp2_frames)})
        assert sorted(sent) == [sc.start_address for sc in plans[s]]
        for k, sc in enumerate(plans[s]):
            got = outs[s][k].cpu().numpy()
            for t in range(15, 4 * fps):
                assert (got[t] == sent[sc.start_address][(t - 15) % 20]).all(), (s, k, t)
