"""dabgpu_dabplus_follow_dev restated in numpy from its contract (include/dabgpu.h), on top of dabplus_reference.superframe
and .firecode: a test helper that shares no code with the library.

One entry in one call.  F = the `held` frames of the carry record followed by the new logical frames, T = len(F).  Frame i
is a raw hit when its first 11 bytes, uncorrected, are not all zero and the Fire code over bytes 2..10 equals bytes 0..1;
votes[r] = hits at i = r (mod 5).  Phase p: with a synced carry 0 unless a residue has strictly more votes than residue 0;
then, and without a synced carry, the smallest residue with the maximum if that is > 0; else none.  No phase: nothing is
emitted, the last min(4, T) frames are carried with synced = 0, the rest is dropped.  With a phase: super-frame k = frames
p + 5k .. p + 5k + 4 for k < (T - p) // 5, p frames dropped, the frames from p + 5 n_sf on carried, synced = 1 iff
votes[p] > 0 or nothing was emitted.  The carry record: int32 {synced, held, 0, 0}, the held frames, zeros up to 16 + 96 s.

Also the streams the tests feed: synth.build_superframe super-frames one after the other, cut at a logical-frame offset,
behind erasure frames (what the channel decoder gives for erased soft bits: zeros, energy-dispersed)."""
import numpy as np

import dabplus_reference as R

RESULT_DTYPE = np.dtype([("n_superframes", np.int32), ("phase", np.int32), ("synced", np.int32), ("dropped", np.int32),
                         ("raw_hits", np.int32), ("held", np.int32), ("reserved", np.int32, (2,))])
CARRY_HEADER = 16


def carry_bytes(s):
    return CARRY_HEADER + 4 * 24 * s                     # (96 s is a multiple of 16 already)


def raw_hit(frame):
    h = np.asarray(frame[:11], np.uint8)
    return bool(h.any()) and R.firecode(h[2:11]) == (int(h[0]) << 8 | int(h[1]))


_SF_CACHE = {}


def superframe(sf, s):
    """dabplus_reference.superframe, remembered per content (the chunked tests decode the same bytes many times)"""
    key = (s, sf.tobytes())
    hit = _SF_CACHE.get(key)
    if hit is None:
        hit = _SF_CACHE[key] = R.superframe(sf, s)
    return hit


def follow(new, s, carry=None):
    """new: uint8 [n_cifs][24 s]; carry: uint8 [carry_bytes(s)] or None -> (data [n_sf][110 s], status [n_sf] R.STATUS_DTYPE,
    result RESULT_DTYPE record, carry_out uint8 [carry_bytes(s)])"""
    lf = 24 * s
    new = np.asarray(new, np.uint8).reshape(-1, lf)
    synced = held = 0
    if carry is not None:
        hdr = np.asarray(carry[:CARRY_HEADER], np.uint8).view("<i4")
        if 0 <= int(hdr[1]) <= 4:
            synced, held = int(hdr[0] != 0), int(hdr[1])
    F = new if held == 0 else np.concatenate([np.asarray(carry[CARRY_HEADER:CARRY_HEADER + held * lf], np.uint8).reshape(held, lf), new])
    T = len(F)
    votes = [0] * 5
    for i in range(T):
        votes[i % 5] += raw_hit(F[i])
    best = max(votes)
    if synced and votes[0] == best:
        p = 0
    elif best > 0:
        p = votes.index(best)
    else:
        p = None
    res = np.zeros((), RESULT_DTYPE)
    res["raw_hits"] = sum(votes)
    if p is None:
        n_sf, first_kept, synced_out = 0, T - min(4, T), 0
        res["phase"], res["dropped"] = -1, first_kept
    else:
        n_sf = (T - p) // 5
        first_kept = p + 5 * n_sf
        synced_out = int(votes[p] > 0 or n_sf == 0)
        res["phase"], res["dropped"] = p, p
    data = np.zeros((n_sf, 110 * s), np.uint8)
    status = np.zeros(n_sf, R.STATUS_DTYPE)
    for k in range(n_sf):
        data[k], status[k] = superframe(F[p + 5 * k:p + 5 * k + 5].reshape(-1), s)
    kept = F[first_kept:]
    assert 0 <= len(kept) <= 4
    out = np.zeros(carry_bytes(s), np.uint8)
    out[:CARRY_HEADER].view("<i4")[:2] = [synced_out, len(kept)]
    out[CARRY_HEADER:CARRY_HEADER + kept.size] = kept.reshape(-1)
    res["n_superframes"], res["synced"], res["held"] = n_sf, synced_out, len(kept)
    return data, status, res, out


def follow_chunks(frames, s, chunks, carry=None):
    """The calls a caller makes for `frames` cut into `chunks` (frame counts; the last one takes what is left), the carry
    handed from each to the next -> list of follow() results."""
    out, at = [], 0
    for n in chunks:
        r = follow(frames[at:at + n], s, carry)
        out.append(r)
        carry = r[3]
        at += n
    return out


def cut(total, size):
    """chunk sizes of `size` covering `total` frames, the last one shorter"""
    return [min(size, total - a) for a in range(0, total, size)]


# ---------------------------------------------------------------------------------------------------------- streams
def dispersal_bytes(n):
    """The first n bytes of the energy-dispersal sequence (EN 300 401 clause 10: x^9 + x^5 + 1, register all ones): what a
    logical frame of erasures decodes to."""
    reg = [1] * 9
    bits = []
    for _ in range(8 * n):
        b = reg[8] ^ reg[4]
        bits.append(b)
        reg = [b] + reg[:8]
    return np.packbits(np.array(bits, np.uint8))


def erasure_frames(n, s):
    return np.tile(dispersal_bytes(24 * s), (n, 1))


def build_stream(seed, bitrate, n_sf, cut_frames=0, lead=0, combo=(1, 0)):
    """-> (frames uint8 [lead + 5 n_sf - cut_frames][24 s], sfs [n_sf][120 s], starts: indices of the start frames).
    `lead` erasure frames, then n_sf super-frames of synth.build_superframe without their first `cut_frames` logical
    frames.  Asserts what every test relies on: every start frame is a raw hit and no other frame is one."""
    from dabgpu import synth
    s = bitrate // 8
    rng = np.random.default_rng(seed)
    sfs = np.stack([synth.build_superframe(rng, bitrate, *combo)[0] for _ in range(n_sf)])
    frames = np.concatenate([erasure_frames(lead, s), sfs.reshape(5 * n_sf, 24 * s)[cut_frames:]])
    starts = [lead + 5 * k - cut_frames for k in range(n_sf) if 5 * k >= cut_frames]
    for i in range(len(frames)):
        assert raw_hit(frames[i]) == (i in starts), ("seed %d: frame %d breaks the streams' condition" % (seed, i))
    return frames, sfs, starts
