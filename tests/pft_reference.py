"""The PFT layer of EDI as include/dabgpu_pft.h states it, in plain Python from the definition: the layout rule, the writer
(RS parity by polynomial division) and the reader's contract (erasures filled by Gaussian elimination over GF(2^8) on the
syndrome equations, so that library and reference share no algorithm).  Imports numpy and nothing of the library."""
import numpy as np

FIRST_ROOT = 1
PARITY, RS_K, MAX_CHUNKS, MAX_FRAGMENTS, MAX_PLEN, MAX_BLOCK, MAX_TAIL = 48, 207, 40, 256, 8192, 10496, 8211
FEC, ADDR, RECOVERED, INCONSISTENT, LOST, AF_OK, FLUSHED = 1, 2, 4, 8, 16, 32, 64
COUNTERS = ("records", "packets", "lost", "recovered", "fragments", "duplicates", "mismatched", "late", "unsupported", "missing",
            "skipped", "resyncs", "out_bytes", "chunks_filled", "bytes_filled")
HEAD_BYTES, GROUP_HEAD_BYTES = 144, 64
GROUP_BYTES = GROUP_HEAD_BYTES + MAX_BLOCK
TAIL_AT = HEAD_BYTES + 2 * GROUP_BYTES
STATE_BYTES = TAIL_AT + 8224
OUT_SLACK = 29216

# ---- GF(2^8), x^8 + x^4 + x^3 + x^2 + 1, alpha = 2
EXP, LOG = [0] * 510, [0] * 256
_x = 1
for _i in range(255):
    EXP[_i], LOG[_x] = _x, _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
for _i in range(255, 510):
    EXP[_i] = EXP[_i - 255]


def mul(a, b):
    return EXP[LOG[a] + LOG[b]] if a and b else 0


def inv(a):
    return EXP[255 - LOG[a]]


def alpha(e):
    return EXP[e % 255]


def generator():
    """prod (x + alpha^(FIRST_ROOT + i)), coefficients from the highest power down"""
    g = [1]
    for i in range(PARITY):
        r = alpha(FIRST_ROOT + i)
        g = [a ^ mul(b, r) for a, b in zip(g + [0], [0] + g)]
    return g


GEN = generator()


def parity(data):
    """the 48 parity bytes of one chunk: the remainder of data(x) x^48 by the generator"""
    rem = list(data) + [0] * PARITY
    for i in range(len(data)):
        c = rem[i]
        if c:
            for j in range(1, PARITY + 1):
                rem[i + j] ^= mul(c, GEN[j])
    return bytes(rem[len(data):])


def evaluate(codeword, e):
    """the codeword (first byte = the highest power) at alpha^e"""
    acc, x = 0, alpha(e)
    for b in codeword:
        acc = mul(acc, x) ^ b
    return acc


def crc16(data):
    crc = 0xFFFF
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc ^ 0xFFFF


# ---- the layout
def block_index(c, k, i, j):
    return i * k + j if j < k else c * k + PARITY * i + (j - k)


def chunk_counts(c, k, f):
    """counts[i][g] = the positions of chunk i that fragment g holds"""
    i, j = np.divmod(np.arange(c * (k + PARITY)), k + PARITY)
    idx = np.where(j < k, i * k + j, c * k + PARITY * i + (j - k))
    return np.bincount(i * f + idx % f, minlength=c * f).reshape(c, f)


def layout(l, fec=True, m=2, max_payload=1400, addr=False):
    """dict, or None where the rule refuses"""
    if not 12 <= l <= 8192 or m < 0 or max_payload < 1:
        return None
    hl = 14 + (2 if fec else 0) + (4 if addr else 0)
    if not fec:
        s = min(max_payload, MAX_PLEN)
        f = -(-l // s)
        if f > MAX_FRAGMENTS:
            return None
        return dict(packet_bytes=l, fec=0, m=m, max_payload=max_payload, addr=int(addr), chunks=0, rs_k=0, rs_z=0, block_bytes=0,
                    fcount=f, plen=s, header_bytes=hl, stream_bytes=f * hl + l, guaranteed_losses=0)
    c = -(-l // RS_K)
    k = -(-l // c)
    B = c * (k + PARITY)
    s0 = min(PARITY * c // (m + 1), max_payload)
    if s0 < 1:
        return None
    for f in range(-(-B // s0), MAX_FRAGMENTS + 1):
        s = -(-B // f)
        if not 1 <= s <= MAX_PLEN or f * s // (k + PARITY) != c:
            if m == 0:
                return None
            continue
        counts = chunk_counts(c, k, f)
        best = f
        for i in range(c):
            worst_first = np.sort(counts[i])[::-1]
            best = min(best, int(np.searchsorted(np.cumsum(worst_first), PARITY, side="right")))
        if best < m:
            continue
        return dict(packet_bytes=l, fec=1, m=m, max_payload=max_payload, addr=int(addr), chunks=c, rs_k=k, rs_z=c * k - l, block_bytes=B,
                    fcount=f, plen=s, header_bytes=hl, stream_bytes=f * (hl + s), guaranteed_losses=best)
    return None


# ---- the writer
def header(pseq, findex, fcount, plen, fec=None, addr=None):
    """fec: (RSk, RSz) or None; addr: (source, dest) or None"""
    h = b"PF" + (pseq & 0xFFFF).to_bytes(2, "big") + findex.to_bytes(3, "big") + fcount.to_bytes(3, "big")
    h += ((0x8000 if fec else 0) | (0x4000 if addr else 0) | plen).to_bytes(2, "big")
    if fec:
        h += bytes(fec)
    if addr:
        h += addr[0].to_bytes(2, "big") + addr[1].to_bytes(2, "big")
    return h + crc16(h).to_bytes(2, "big")


def rs_block(af, a):
    c, k = a["chunks"], a["rs_k"]
    data = bytes(af) + bytes(a["rs_z"])
    return data + b"".join(parity(data[i * k:(i + 1) * k]) for i in range(c))


def fragments(af, a, pseq, source=0, dest=0):
    """one AF packet -> the list of its fragments, headers included"""
    f, s = a["fcount"], a["plen"]
    addr = (source, dest) if a["addr"] else None
    if not a["fec"]:
        return [header(pseq, g, f, len(af[g * s:(g + 1) * s]), None, addr) + bytes(af[g * s:(g + 1) * s]) for g in range(f)]
    block = rs_block(af, a) + bytes(f * s - a["block_bytes"])
    return [header(pseq, g, f, s, (a["rs_k"], a["rs_z"]), addr) + block[g::f][:s] for g in range(f)]


# ---- the reader
def parse_header(s, q):
    """(status, fields): 2 = T, 1 = the walk stops (incomplete fragment or cut header), 0 = neither"""
    avail = len(s) - q
    if avail < 12:
        return 1, None
    if s[q:q + 2] != b"PF":
        return 0, None
    w = int.from_bytes(s[q + 10:q + 12], "big")
    fec, addr, plen = w >> 15, (w >> 14) & 1, w & 0x3FFF
    hl = 14 + 2 * fec + 4 * addr
    if avail < hl:
        return 1, None
    h = dict(pseq=int.from_bytes(s[q + 2:q + 4], "big"), findex=int.from_bytes(s[q + 4:q + 7], "big"),
             fcount=int.from_bytes(s[q + 7:q + 10], "big"), fec=fec, addr=addr, plen=plen, rs_k=0, rs_z=0, source=0, dest=0, hl=hl)
    at = q + 12
    if fec:
        h["rs_k"], h["rs_z"] = s[at], s[at + 1]
        at += 2
    if addr:
        h["source"], h["dest"] = int.from_bytes(s[at:at + 2], "big"), int.from_bytes(s[at + 2:at + 4], "big")
        at += 4
    if not (1 <= h["fcount"] <= 256 and h["findex"] < h["fcount"] and 1 <= plen <= 8192 and (not fec or 1 <= h["rs_k"] <= 207)):
        return 0, None
    if crc16(s[q:at]) != int.from_bytes(s[at:at + 2], "big"):
        return 0, None
    return (2 if hl + plen <= avail else 1), h


NP_EXP, NP_LOG = np.array(EXP, np.int64), np.array(LOG, np.int64)


def np_mul(a, b):
    """element by element over GF(2^8), on integer arrays"""
    return np.where((a != 0) & (b != 0), NP_EXP[NP_LOG[a] + NP_LOG[b]], 0)


def syndromes(codeword, count):
    """the codeword at alpha^FIRST_ROOT .. alpha^(FIRST_ROOT + count - 1): sum of byte j times alpha^(root (n - 1 - j))"""
    cw = np.asarray(codeword, np.int64)
    power = (np.arange(FIRST_ROOT, FIRST_ROOT + count)[:, None] * (len(cw) - 1 - np.arange(len(cw)))[None, :]) % 255
    terms = np.where(cw[None, :] != 0, NP_EXP[NP_LOG[cw][None, :] + power], 0)
    return np.bitwise_xor.reduce(terms, axis=1)


def solve(rows, rhs):
    """Gaussian elimination over GF(2^8): the unique x with rows x = rhs"""
    n = len(rhs)
    a = np.concatenate([np.asarray(rows, np.int64).reshape(n, n), np.asarray(rhs, np.int64).reshape(n, 1)], axis=1)
    for col in range(n):
        piv = col + int(np.nonzero(a[col:, col])[0][0])
        a[[col, piv]] = a[[piv, col]]
        a[col] = np_mul(a[col], np.full(n + 1, inv(int(a[col, col])), np.int64))
        factors = a[:, col].copy()
        factors[col] = 0
        a ^= np_mul(factors[:, None], a[col][None, :])
    return a[:, n]


def fill(codeword, erased):
    """codeword: list of k + 48 bytes, the erased positions zero -> (filled, consistent)"""
    n, e = len(codeword), len(erased)
    rows = [[alpha((FIRST_ROOT + i) * (n - 1 - p)) for p in erased] for i in range(e)]
    out = list(codeword)
    for p, v in zip(erased, solve(rows, syndromes(codeword, e))):
        out[p] = int(v)
    return out, not syndromes(out, PARITY).any()


def af_ok(p):
    return (len(p) >= 12 and p[:2] == b"AF" and int.from_bytes(p[2:6], "big") + 12 == len(p) <= 8192 and p[8] & 0xF0 == 0x90 and
            p[9:10] == b"T" and crc16(p[:-2]) == int.from_bytes(p[-2:], "big"))


def new_state():
    return dict(have=False, horizon=0, late_run=0, in_skip=False, tail=b"", groups={}, totals={k: 0 for k in COUNTERS})


def fec_view(fcount, s, k, z):
    if fcount * s > MAX_BLOCK:
        return None
    c = fcount * s // (k + PARITY)
    if not 1 <= c <= MAX_CHUNKS or not 12 <= c * k - z <= 8192:
        return None
    return c, c * k - z


def read(state, data, flush=False):
    """One call of one entry.  state: new_state() or what an earlier call returned (not changed).
    -> (records [dict], output bytes, result dict, the new state)"""
    st = dict(state, groups={p: dict(g, frags=dict(g["frags"])) for p, g in state["groups"].items()}, totals=dict(state["totals"]))
    s = bytes(st["tail"][:MAX_TAIL]) + bytes(data)
    c = {k: 0 for k in COUNTERS}
    records, out = [], bytearray()

    def holds(p):
        g = st["groups"].get(p)
        return g is not None and g["kind"] == 1 and len(g["frags"]) > 0

    def close(p, extra=0, counted=True):
        g = st["groups"].pop(p, None)
        if g is None or g["kind"] != 1 or not g["frags"]:
            if counted:
                c["missing"] += 1
            return
        f, have = g["fcount"], g["frags"]
        flags = extra | (FEC if g["fec"] else 0) | (ADDR if g["addr"] else 0)
        packet, worst = None, 0
        if len(have) == f:
            if g["fec"]:
                packet = b"".join(bytes(x) for x in zip(*[have[i] for i in range(f)]))[:g["length"]]
            else:
                packet = b"".join(have[i] for i in range(f))
        elif g["fec"]:
            k, n_chunks, n = g["rs_k"], g["chunks"], g["rs_k"] + PARITY
            block = [have[i % f][i // f] if i % f in have else None for i in range(n_chunks * n)]
            chunks, filled, erased_total, clean = [], 0, 0, True
            for i in range(n_chunks):
                cw = [block[block_index(n_chunks, k, i, j)] for j in range(n)]
                erased = [j for j, v in enumerate(cw) if v is None]
                worst = max(worst, len(erased))
                chunks.append((cw, erased))
            if worst <= PARITY:
                data_bytes = bytearray()
                for cw, erased in chunks:
                    if erased:
                        cw, ok = fill([0 if v is None else v for v in cw], erased)
                        clean, filled, erased_total = clean and ok, filled + 1, erased_total + len(erased)
                    data_bytes += bytes(cw[:k])
                packet = bytes(data_bytes[:g["length"]])
                flags |= RECOVERED | (0 if clean else INCONSISTENT)
                c["recovered"] += 1
                c["chunks_filled"] += filled
                c["bytes_filled"] += erased_total
        if packet is None:
            flags |= LOST
            c["lost"] += 1
            packet = b""
        else:
            c["packets"] += 1
            if af_ok(packet):
                flags |= AF_OK
        records.append(dict(offset=len(out), length=len(packet), pseq=p, fcount=f, received=len(have), plen=g["s"] or 0, rs_k=g["rs_k"],
                            rs_z=g["rs_z"], chunks=g["chunks"], max_erasures=min(worst, 255), flags=flags, source=g["source"], dest=g["dest"]))
        out.extend(packet)
        c["records"] += 1

    def join(h, payload):
        p = h["pseq"]
        g = st["groups"].get(p)
        if g is None:
            g = dict(kind=1, fcount=h["fcount"], fec=h["fec"], addr=h["addr"], rs_k=h["rs_k"], rs_z=h["rs_z"], source=h["source"],
                     dest=h["dest"], s=None, chunks=0, length=0, frags={})
            if h["fec"]:
                view = fec_view(h["fcount"], h["plen"], h["rs_k"], h["rs_z"])
                if view is None:
                    g = dict(kind=2, frags={})
                else:
                    g["s"], (g["chunks"], g["length"]) = h["plen"], view
            st["groups"][p] = g
        if g["kind"] == 2:
            c["unsupported"] += 1
            return
        same = all(h[k] == g[k] for k in ("fcount", "fec", "addr", "rs_k", "rs_z", "source", "dest")) and (not g["fec"] or h["plen"] == g["s"])
        if not same:
            c["mismatched"] += 1
            return
        if h["findex"] in g["frags"]:
            c["duplicates"] += 1
            return
        if not g["fec"]:
            last = h["findex"] == g["fcount"] - 1
            if last:
                if g["s"] is not None and h["plen"] > g["s"]:
                    c["mismatched"] += 1
                    return
                if g["fcount"] == 1:
                    g["s"] = h["plen"]
            elif g["s"] is None:
                held_last = g["frags"].get(g["fcount"] - 1)
                if held_last is not None and len(held_last) > h["plen"]:
                    c["mismatched"] += 1
                    return
                if h["fcount"] * h["plen"] > MAX_BLOCK:
                    st["groups"][p] = dict(kind=2, frags={})
                    c["unsupported"] += 1
                    return
                g["s"] = h["plen"]
            elif h["plen"] != g["s"]:
                c["mismatched"] += 1
                return
        g["frags"][h["findex"]] = bytes(payload)

    p, n = 0, len(s)
    in_skip = st["in_skip"]
    while True:
        q, status, h = p, 0, None
        while q < n:
            status, h = parse_header(s, q)
            if status:
                break
            q += 1
        if q > p:
            c["skipped"] += q - p
            in_skip = True
            p = q
        if p >= n or status != 2:
            break
        if in_skip:
            c["resyncs"] += 1
            in_skip = False
        c["fragments"] += 1
        seq = h["pseq"]
        if not st["have"]:
            st["have"], st["horizon"] = True, (seq - 1) & 0xFFFF
        d = (seq - st["horizon"]) & 0xFFFF
        late = d == 0 or d >= 32768
        if late and st["late_run"] < 16:
            st["late_run"] += 1
            c["late"] += 1
        else:
            if late:
                for dist in (1, 2):
                    pq = (st["horizon"] + dist) & 0xFFFF
                    if holds(pq):
                        close(pq)
                    else:
                        st["groups"].pop(pq, None)
                st["horizon"], d = (seq - 1) & 0xFFFF, 1
            st["late_run"] = 0
            if d >= 3:
                for dist in (1, 2):
                    if dist <= d - 2:
                        close((st["horizon"] + dist) & 0xFFFF)
                c["missing"] += max(d - 4, 0)
                st["horizon"] = (seq - 2) & 0xFFFF
            join(h, s[p + h["hl"]:p + h["hl"] + h["plen"]])
            while True:
                nxt = (st["horizon"] + 1) & 0xFFFF
                g = st["groups"].get(nxt)
                if g is None or g["kind"] != 1 or len(g["frags"]) != g["fcount"]:
                    break
                close(nxt)
                st["horizon"] = nxt
        p += h["hl"] + h["plen"]
    if flush and st["have"]:
        p1, p2 = (st["horizon"] + 1) & 0xFFFF, (st["horizon"] + 2) & 0xFFFF
        h1, h2 = holds(p1), holds(p2)
        if h1:
            close(p1, FLUSHED)
        if h2:
            if not h1:
                close(p1)
            close(p2, FLUSHED)
        st["horizon"] = (st["horizon"] + (2 if h2 else 1 if h1 else 0)) & 0xFFFF
    st["in_skip"], st["tail"] = in_skip, s[p:]
    c["out_bytes"] = len(out)
    for k in COUNTERS:
        st["totals"][k] += c[k]
    return records, bytes(out), dict(c, tail_bytes=n - p), st


# ---- the state record of the library, from the reference's state
HEAD_DTYPE = np.dtype([("tail_bytes", "<u4"), ("have_horizon", "u1"), ("in_skip", "u1"), ("late_run", "u1"), ("reserved", "u1"),
                       ("horizon", "<u2"), ("reserved1", "<u2"), ("reserved2", "<u4")] +
                      [(k, "<u8") for k in COUNTERS] + [("reserved3", "<u8")])
GROUP_DTYPE = np.dtype([("kind", "u1"), ("fec", "u1"), ("addr", "u1"), ("have_s", "u1"), ("pseq", "<u2"), ("fcount", "<u2"), ("s", "<u2"),
                        ("last_len", "<u2"), ("received", "<u2"), ("source", "<u2"), ("dest", "<u2"), ("length", "<u2"), ("rs_k", "u1"),
                        ("rs_z", "u1"), ("chunks", "u1"), ("reserved", "u1"), ("reserved1", "<u4"), ("reserved2", "<u4"), ("map", "<u8", (4,))])
assert HEAD_DTYPE.itemsize == HEAD_BYTES and GROUP_DTYPE.itemsize == GROUP_HEAD_BYTES


def pack_state(st):
    """the STATE_BYTES record the library leaves for this state"""
    rec = np.zeros(STATE_BYTES, np.uint8)
    head = rec[:HEAD_BYTES].view(HEAD_DTYPE)[0]
    head["tail_bytes"], head["have_horizon"], head["in_skip"], head["late_run"] = len(st["tail"]), st["have"], st["in_skip"], st["late_run"]
    head["horizon"] = st["horizon"] if st["have"] else 0
    for k in COUNTERS:
        head[k] = st["totals"][k]
    for p, g in st["groups"].items():
        at = HEAD_BYTES + (p & 1) * GROUP_BYTES
        gh = rec[at:at + GROUP_HEAD_BYTES].view(GROUP_DTYPE)[0]
        buf = rec[at + GROUP_HEAD_BYTES:at + GROUP_BYTES]
        gh["kind"], gh["pseq"] = g["kind"], p
        if g["kind"] != 1:
            continue
        for k in ("fec", "addr", "fcount", "source", "dest", "length", "rs_k", "rs_z", "chunks"):
            gh[k] = g[k]
        gh["have_s"], gh["s"], gh["received"] = g["s"] is not None, g["s"] or 0, len(g["frags"])
        bits = 0
        for i, payload in g["frags"].items():
            bits |= 1 << i
            if not g["fec"] and i == g["fcount"] - 1:
                gh["last_len"] = len(payload)
                buf[MAX_BLOCK - len(payload):] = np.frombuffer(payload, np.uint8)
            else:
                buf[i * g["s"]:i * g["s"] + len(payload)] = np.frombuffer(payload, np.uint8)
        gh["map"] = [(bits >> (64 * w)) & (2 ** 64 - 1) for w in range(4)]
    rec[TAIL_AT:TAIL_AT + len(st["tail"])] = np.frombuffer(st["tail"], np.uint8)
    return rec
