"""The from-definition DAB+ reference (tests/dabplus_reference.py) checked on its own, and the CPU oracle checked against it
column by column: the oracle's RS decoder is the HIP kernel's algorithm line for line, so agreeing with each other
proves little; both must agree with a decoder built another way (Peterson-Gorenstein-Zierler, no Berlekamp-Massey, no
Forney), including on inputs beyond the code's reach."""
import numpy as np

import dabplus_reference as R
from oracle import oracle as O


def _codeword(rng):
    return R.rs_encode(rng.integers(0, 256, R.K, dtype=np.uint8))


def _hit(cw, positions, rng):
    e = cw.copy()
    e[list(positions)] ^= rng.integers(1, 256, len(positions), dtype=np.uint8)
    return e


def test_field_and_code_from_their_definitions():
    assert R.gf_mul_bits(0x80, 2) == 0x1D and sorted(R.EXP.tolist()) == list(range(1, 256))
    for a in range(1, 256):
        assert R.gmul(a, R.ginv(a)) == 1
    rng = np.random.default_rng(20)
    cw = R.rs_encode(rng.integers(0, 256, (64, R.K), dtype=np.uint8))
    assert not R.syndromes(cw).any()
    # the generator prod (x + alpha^k) divides every codeword: the same code as the oracle's systematic encoder
    for c in cw[:4]:
        assert (c[R.K:] == O.rs_encode(c[:R.K])).all()


def test_reference_corrects_up_to_five_errors_at_the_edges():
    rng = np.random.default_rng(21)
    for pos in R.EDGE_ERROR_POSITIONS:
        for _ in range(3):
            cw = _codeword(rng)
            got = R.rs_decode(_hit(cw, pos, rng))
            assert got is not None and got[1] == len(pos) and (got[0] == cw).all(), pos


def test_reference_miscorrects_to_the_codeword_within_distance_five():
    rng = np.random.default_rng(22)
    for _ in range(40):
        cw = _codeword(rng)
        r, other = R.forced_miscorrection(cw, rng)
        assert (r != cw).sum() == 6 and (r != other).sum() == 5
        got = R.rs_decode(r)
        assert got is not None and got[1] == 5 and (got[0] == other).all()


def test_reference_outputs_are_codewords_within_distance_five():
    rng = np.random.default_rng(23)
    n_fail = 0
    for ne in range(0, 11):
        for _ in range(30):
            r = _hit(_codeword(rng), rng.choice(R.N, ne, replace=False), rng)
            got = R.rs_decode(r)
            if got is None:
                assert ne > 5
                n_fail += 1
                continue
            assert not R.syndromes(got[0]).any() and (got[0] != r).sum() == got[1] <= 5
    assert n_fail > 100                                                # random words beyond t are almost never decodable


def _columns(rng):
    """A few thousand columns: 0..10 random errors, the edge patterns, forced miscorrections, all-0xFF and all-zero."""
    cols = []
    for ne in range(0, 11):
        for _ in range(220):
            cols.append(_hit(_codeword(rng), rng.choice(R.N, ne, replace=False), rng))
    for pos in R.EDGE_ERROR_POSITIONS:
        cols.append(_hit(_codeword(rng), pos, rng))
    for _ in range(300):
        cols.append(R.forced_miscorrection(_codeword(rng), rng)[0])
    cols += [np.full(R.N, 0xFF, np.uint8), np.zeros(R.N, np.uint8)]
    return cols


def test_oracle_rs_decoder_equals_the_reference():
    """Same bytes, same count, same flag -- also beyond t = 5, where a bounded-distance decoder must either find the one
    codeword within distance 5 or flag the column and leave it alone."""
    rng = np.random.default_rng(24)
    n_mis = 0
    for i, r in enumerate(_columns(rng)):
        want = R.rs_decode(r)
        c, n = O.rs_decode(r)
        if want is None:
            assert n == -1 and (c == r).all(), i
        else:
            assert n == want[1] and (c == want[0]).all(), i
            n_mis += n == 5 and (r != want[0]).sum() == 5
    assert n_mis >= 300
