"""The EDI stream walk from the contract (include/dabgpu_edi.h, "THE CONTRACT"), in plain Python over tests/edi_reference.py:
what one entry of dabgpu_edi_read_host must leave in one call.  Shares no code with the header."""
import edi_reference as P
from dabgpu.synth import crc16

GAP, SEQ_BREAK, FP_MISMATCH, STAT_FIELD, FIB_CRC, NO_FIC, TIME = 1, 2, 4, 8, 16, 32, 64


def new_state():
    return {"tail": b"", "prev": None, "seq": None, "in_skip": False}


def good(S, q):
    """C of the contract: the packet's length, or None"""
    total = P.header(S, q)
    if total is None or q + total > len(S):
        return None
    return total if crc16(S[q:q + total - 2]) == int.from_bytes(S[q + total - 2:q + total], "big") else None


def plan_key(streams):
    import eti_reference as E
    return [(st["id"], st["start"], E.tpl_of(st), E.stl_of(st)) for st in E.ordered(streams)]


def read(state, new, plan=None):
    """state: new_state() or what an earlier call returned; new: bytes; plan: None (discovery) or the stream dicts.
    -> (rows [{fic, crc_ok, data [per plan stream], status dict}], counters dict, state)"""
    S = state["tail"][:8191] + bytes(new)
    prev, seq_prev, in_skip = state["prev"], state["seq"], state["in_skip"]
    key = None if plan is None else plan_key(plan)
    c = dict(rows=0, not_deti=0, bad_tags=0, other_plan=0, skipped=0, resyncs=0, gap_sum=0, fib_errors=0)
    rows, p = [], 0
    while True:
        total = good(S, p)
        if total is None:
            q = next((q for q in range(p + 1, len(S) - 9) if good(S, q) is not None), None)
            if q is None:
                t = next((t for t in range(p, len(S) - 9) if (P.header(S, t) or 0) + t > len(S)), max(p, len(S) - 9))
                if t > p:
                    c["skipped"] += t - p
                    in_skip = True
                p = t
                break
            c["skipped"] += q - p
            in_skip = True
            p, total = q, good(S, q)
        if in_skip:
            c["resyncs"] += 1
            in_skip = False
        pkt = S[p:p + total]
        seq = int.from_bytes(pkt[6:8], "big")
        seq_break = seq_prev is not None and seq != (seq_prev + 1) % 65536
        seq_prev = seq
        try:
            d = P.parse_payload(pkt[10:-2])
        except P.Malformed:
            c["bad_tags"] += 1
            d = None
        except P.NotDeti:
            c["not_deti"] += 1
            d = None
        if d is not None and key is not None and [(s["scid"], s["sad"], s["tpl"], s["stl"]) for s in d["streams"]] != key:
            c["other_plan"] += 1
            d = None
        if d is not None:
            fic = d["fic"] if d["ficf"] else bytes(96)
            ok = [int(bool(d["ficf"]) and crc16(fic[32 * j:32 * j + 30]) == int.from_bytes(fic[32 * j + 30:32 * j + 32], "big"))
                  for j in range(3)]
            fib_ok = ok[0] | ok[1] << 1 | ok[2] << 2
            gap = 0 if prev is None else (d["dlfc"] - prev - 1) % 5000
            flags = (GAP if gap else 0) | (SEQ_BREAK if seq_break else 0) | (FP_MISMATCH if d["fp"] != d["dlfc"] % 8 else 0) | \
                (STAT_FIELD if d["stat"] != 0xFF else 0) | (FIB_CRC if d["ficf"] and fib_ok != 7 else 0) | \
                (0 if d["ficf"] else NO_FIC) | (TIME if d["atstf"] else 0)
            status = dict(offset=p, length=total, dlfc=d["dlfc"], seq=seq, gap=gap, fp=d["fp"], stat=d["stat"], mid=d["mid"],
                          fib_ok=fib_ok, flags=flags, utco=d["utco"], seconds=d["seconds"], tsta=d["tsta"])
            rows.append({"fic": fic, "crc_ok": ok, "data": [s["data"] for s in d["streams"]] if key is not None else [],
                         "status": status})
            c["rows"] += 1
            c["gap_sum"] += gap
            if d["ficf"]:
                c["fib_errors"] += 3 - sum(ok)
            prev = d["dlfc"]
        p += total
    c["tail_bytes"] = len(S) - p
    return rows, c, {"tail": S[p:], "prev": prev, "seq": seq_prev, "in_skip": in_skip}
