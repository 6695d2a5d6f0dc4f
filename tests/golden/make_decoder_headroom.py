#!/usr/bin/env python3
"""Generates tests/golden/decoder_headroom.npz: decoder inputs (606 trellis steps of the unpunctured mother code) found
by a seeded search for a large path-metric excursion, as tests/decoder_reference.py measures it (the distance of any
path metric from the state-0 metric at the last multiple of 12 steps: what a decoder with 16-bit metrics that
renormalises every 12 steps has to hold).  The search starts from a transmitted codeword at +-127 and keeps random
changes -- a burst of message bits replaced, a burst of steps inverted, erased or restored -- whenever the excursion
does not fall.  The file holds soft bits and the reference's figures of them; nothing else.

    python tests/golden/make_decoder_headroom.py            # about two minutes
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "sdrplusplus-dab-radio-plugin_amd"))
import decoder_reference as R      # noqa: E402

NSTEPS = 606                 # 600 information bits: whole bytes
N_INPUTS = 12
ROUNDS = 120
CANDIDATES = 48


def render(msg, gain):
    """The codeword of msg at +-127, every soft bit multiplied by its gain (1, -1 = inverted, 0 = erased)."""
    return (R.conv_encode(msg)[0].astype(np.int64) * 2 - 1) * 127 * gain


def propose(rng, msg, gain):
    """One random change: a burst of 1 .. 16 steps of the message or of the gains."""
    msg, gain = msg.copy(), gain.copy()
    n = int(rng.integers(1, 17))
    kind = int(rng.integers(0, 6))
    if kind < 3:                                                                 # the message: other bits, ones, zeros
        t = int(rng.integers(0, msg.size - n + 1))
        msg[t:t + n] = rng.integers(0, 2, n) if kind == 0 else (kind - 1)
    else:
        t = int(rng.integers(0, NSTEPS - n + 1))
        span = slice(4 * t, 4 * (t + n))
        if kind == 3:
            gain[span] = -gain[span]                                             # inverted burst
        elif kind == 4:
            gain[span] = 0                                                       # erased
        else:
            gain[span] = 1                                                       # as transmitted again
    return msg, gain


def search(seed):
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 2, NSTEPS - 6, dtype=np.uint8)
    gain = np.ones(4 * NSTEPS, np.int64)
    score = int(R.viterbi(render(msg, gain)).excursion[0])
    start = score
    for _ in range(ROUNDS):
        cand = [propose(rng, msg, gain) for _ in range(CANDIDATES)]
        exc = R.viterbi(np.stack([render(m, g) for m, g in cand])).excursion
        k = int(exc.argmax())
        if exc[k] >= score:
            (msg, gain), score = cand[k], int(exc[k])
    return render(msg, gain).astype(np.int8), start, score


def main():
    soft, first = [], []
    for k in range(N_INPUTS):
        x, start, score = search(0xDEC0DE + k)
        print("input %2d: excursion %5d -> %5d" % (k, start, score), flush=True)
        soft.append(x)
        first.append(start)
    soft = np.stack(soft)
    d = R.viterbi(soft)
    np.savez_compressed(os.path.join(HERE, "decoder_headroom.npz"), soft=soft, excursion=d.excursion, spread=d.spread,
                        best=d.best, unique=d.unique, excursion_of_start=np.array(first, np.int64))
    print("largest excursion %d (doubled %d), largest spread %d" % (d.excursion.max(), 2 * d.excursion.max(), d.spread.max()))


if __name__ == "__main__":
    main()
