"""The ETI(NI) reader from its definition (include/dabgpu.h, "ETI(NI) input"; include/dabgpu_eti_read.h, the contract), in
plain Python on `bytes`.  The frame checks are eti_reference.read_frame's; nothing is shared with the library.

A plan is the list of stream dicts eti_reference takes, or None (discovery).  A state is a dict {tail: bytes, have_prev,
last_fct, last_fp, totals: {name: int}}; None = a stream that starts.
"""
import eti_reference as R
from dabgpu.synth import crc16

FRAME = 6144
TAKEN, BAD_SYNC, BAD_HEADER, BAD_HEADER_CRC, BAD_DATA_CRC, OTHER_PLAN = 0, 1, 2, 3, 4, 5
GAP, FP_BREAK, ERR_FIELD, FIB_CRC = 1, 2, 4, 8
COUNTERS = ("rows", "taken", "bad_data_crc", "other_plan", "skipped", "resyncs", "gap_sum", "fib_errors")
_WHY = {"fsync": BAD_SYNC, "header": BAD_HEADER, "fl": BAD_HEADER, "header crc": BAD_HEADER_CRC, "data crc": BAD_DATA_CRC}


def fresh_state():
    return {"tail": b"", "have_prev": False, "last_fct": 0, "last_fp": 0, "totals": dict.fromkeys(COUNTERS, 0)}


def verdict(frame, plan):
    """-> (verdict, info or None).  info is read_frame's dict for verdicts 0 and 5; for 4 the header's fields alone."""
    f = bytes(frame)
    assert len(f) == FRAME
    try:
        if f[4] >= 250:                                     # dabgpu_eti_parse counts an FCT of 250.. as a wrong sync
            raise ValueError("fsync")
        info = R.read_frame(f)
    except ValueError as e:
        v = _WHY[str(e)]
        if v != BAD_DATA_CRC:
            return v, None
        return v, {"err": f[0], "fct": f[4], "fp": f[6] >> 5}
    if plan is not None:
        want = [(st["id"], st["start"], R.tpl_of(st), R.stl_of(st)) for st in R.ordered(plan)]
        got = [(s["scid"], s["sad"], s["tpl"], s["stl"]) for s in info["streams"]]
        if info["nst"] != len(want) or info["fl"] != R.frame_length(plan)[0] or got != want:
            return OTHER_PLAN, info
    return TAKEN, info


def is_candidate(frame):
    return verdict(frame, None)[0] in (TAKEN, BAD_DATA_CRC)


def _next_candidate(s, p):
    """The smallest candidate q with p < q <= len(s) - 6144, or None.  (A candidate has one of the two FSYNC patterns at
    q + 1: only those positions need the full check.)"""
    last = len(s) - FRAME
    q = p
    while True:
        hits = [x for x in (s.find(R.FSYNC_EVEN, q + 2), s.find(R.FSYNC_ODD, q + 2)) if x >= 0]
        if not hits or min(hits) - 1 > last:
            return None
        q = min(hits) - 1
        if is_candidate(s[q:q + FRAME]):
            return q


def read(state, new_bytes, plan):
    """One entry, one call -> (rows, result, state).  A row is a dict {offset, verdict, fct, fp, err, fib_ok, gap, flags,
    fic (96 bytes), crc_ok [3], data {stream id: bytes}}: fic, crc_ok and data are zero unless the row is taken."""
    st = fresh_state() if state is None else state
    s = bytes(st["tail"]) + bytes(new_bytes)
    assert len(st["tail"]) <= FRAME - 1
    have, fct, fp = st["have_prev"], st["last_fct"], st["last_fp"]
    c = dict.fromkeys(COUNTERS, 0)
    rows, p = [], 0
    while p + FRAME <= len(s):
        v, info = verdict(s[p:p + FRAME], plan)
        if v in (TAKEN, BAD_DATA_CRC, OTHER_PLAN):
            row = {"offset": p, "verdict": v, "fct": info["fct"], "fp": info["fp"], "err": info["err"]}
            taken = v == TAKEN
            row["fic"] = info["fic"] if taken else bytes(96)
            fibs = [row["fic"][32 * j:32 * j + 32] for j in range(3)]
            row["crc_ok"] = [int(taken and crc16(b[:30]) == int.from_bytes(b[30:], "big")) for b in fibs]
            row["fib_ok"] = sum(k << j for j, k in enumerate(row["crc_ok"]))
            row["data"] = {}
            if plan is not None:
                for k, sd in enumerate(R.ordered(plan)):
                    row["data"][sd["id"]] = info["streams"][k]["data"] if taken else bytes(8 * R.stl_of(sd))
            row["gap"] = (row["fct"] - (fct + 1)) % 250 if have else 0
            row["flags"] = (GAP if row["gap"] else 0) | (FP_BREAK if have and row["fp"] != (fp + 1) % 8 else 0) | \
                (ERR_FIELD if row["err"] != 0xFF else 0) | (FIB_CRC if taken and row["fib_ok"] != 7 else 0)
            have, fct, fp = True, row["fct"], row["fp"]
            c["rows"] += 1
            c["taken"] += taken
            c["bad_data_crc"] += v == BAD_DATA_CRC
            c["other_plan"] += v == OTHER_PLAN
            c["gap_sum"] += row["gap"]
            c["fib_errors"] += 3 - sum(row["crc_ok"]) if taken else 0
            rows.append(row)
            p += FRAME
            continue
        q = _next_candidate(s, p)
        if q is not None:
            c["skipped"] += q - p
            c["resyncs"] += 1
            p = q
        else:
            c["skipped"] += max(0, len(s) - (FRAME - 1) - p)
            p = max(p, len(s) - (FRAME - 1))
            break
    assert len(rows) <= (FRAME - 1 + len(new_bytes)) // FRAME
    result = dict(c, tail_bytes=len(s) - p)
    new = {"tail": s[p:], "have_prev": have, "last_fct": fct, "last_fp": fp,
           "totals": {k: st["totals"][k] + c[k] for k in COUNTERS}}
    return rows, result, new
