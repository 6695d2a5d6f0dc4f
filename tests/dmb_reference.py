"""T-DMB stream-mode sub-channels from the definition: the contract at the top of include/dabgpu_dmb.h read clause by clause
into Python -- a test transmitter (TS packets, RS(204,188) encoder by polynomial division, the convolutional interleaver as
twelve FIFOs, logical frames) and a serial receiver (sync state machine byte by byte, the de-interleaver as twelve FIFOs of
the complementary depths, the outer code, continuity and census).  No code shared with the header, the kernels or the
library; the GF(2^8) arithmetic and the verified-by-definition decoder are tests/packet_fec_reference.py's.

The library de-interleaves by the closed form x[i] = y[s + 204 (i mod 12) + i]; nothing here does: both FIFO banks are
built from "branch j holds 17 j cells and is visited every 12 bytes".

    frames = to_frames(interleave(encode(packets)), bitrate)        # packets [n][188] uint8
    rx = Receiver(bitrate)                                          # a fresh start; it is the state between calls
    ts, records, counts = rx.call(frames)                           # ts [m][188], records RECORD_DTYPE, counts dict
"""
from collections import deque

import numpy as np

import packet_fec_reference as F

SYNC, CODED, TS, BRANCHES, CELLS = 0x47, 204, 188, 12, 17
LOCK_RUN, LOSS_MISSES = 5, 8
NULL_PID = 0x1FFF
RECORD_DTYPE = np.dtype([("status", np.uint8), ("corrected_data", np.uint8), ("corrected_parity", np.uint8), ("byte3", np.uint8),
                         ("pid", np.uint16), ("flags", np.uint8), ("reserved", np.uint8), ("position", np.uint32),
                         ("reserved2", np.uint32)])
COUNTERS = ("cifs", "bytes", "sync_hits", "locks", "lock_losses", "packets_emitted", "packets_clean", "packets_corrected",
            "packets_uncorrectable", "packets_dropped", "bytes_corrected", "parity_bytes_corrected", "discontinuities", "duplicates")


# ---------------------------------------------------------------- transmitter
def ts_packet(pid, cc, payload=b"", afc=1, af=None, tsc=0, pusi=0, fill=0xFF):
    """One 188-byte TS packet.  afc: adaptation_field_control (1 payload, 2 adaptation field, 3 both); af: the adaptation
    field's bytes after its length byte (None: none; with afc 2 it is stuffed to fill the packet)."""
    head = bytes([SYNC, (pusi << 6) | (pid >> 8), pid & 0xFF, (tsc << 6) | (afc << 4) | (cc & 15)])
    body = b""
    if afc & 2:
        af = b"" if af is None else bytes(af)
        if afc == 2:
            af = af + bytes([0xFF]) * (183 - len(af)) if af else bytes([0x00]) + bytes([0xFF]) * 182
        body = bytes([len(af)]) + af
    if afc & 1:
        body += bytes(payload)
    assert len(body) <= 184
    return np.frombuffer(head + body + bytes([fill]) * (184 - len(body)), np.uint8)


class TsGenerator:
    """Packets of several PIDs, each with its own counter, from a seeded generator."""

    def __init__(self, seed, pids=(0x000, 0x100, 0x111, 0x112, 0x113), null_every=7):
        self.rng = np.random.default_rng(seed)
        self.pids, self.cc, self.null_every, self.n = list(pids), {}, null_every, 0

    def next(self, pid=None, afc=1, af=None, tsc=0, advance=True):
        self.n += 1
        if pid is None:
            pid = NULL_PID if self.null_every and self.n % self.null_every == 0 else self.pids[int(self.rng.integers(len(self.pids)))]
        cc = self.cc.get(pid, int(self.rng.integers(16)) - 1)
        if (afc & 1) and advance and pid != NULL_PID:
            cc = (cc + 1) & 15
        self.cc[pid] = cc & 15
        room = 184 - ((1 + (len(af) if af else (183 if afc == 2 else 0))) if afc & 2 else 0)
        payload = self.rng.integers(0, 256, max(room, 0), dtype=np.uint8).tobytes() if afc & 1 else b""
        payload = payload.replace(bytes([SYNC]), b"\x46")             # no sync byte in payload: the tests plant their own
        return ts_packet(pid, cc & 15, payload, afc, af, tsc)

    def packets(self, n):
        return np.stack([self.next() for _ in range(n)])


def generator_poly():
    g = [1]
    for i in range(16):
        g = F.poly_mul(g, [F.power(2, i), 1])
    return g                                                          # g[k] the coefficient of x^k, g[16] = 1


def encode(packets):
    """[n][188] -> [n][204]: systematic, the parity is the remainder of data(x) x^16 by the generator (all rows at once)"""
    packets = np.asarray(packets, np.uint8)
    g = np.array(generator_poly()[:16], np.uint16)[::-1]              # coefficients of x^15 .. x^0
    reg = np.zeros((len(packets), 16), np.uint16)
    for c in range(TS):
        fb = reg[:, 0] ^ packets[:, c]
        reg = np.concatenate([reg[:, 1:], np.zeros((len(packets), 1), np.uint16)], axis=1)
        reg ^= F.vmul(fb[:, None], g[None, :])
    return np.concatenate([packets, reg.astype(np.uint8)], axis=1)


def interleave(coded, fill=0):
    """[n][204] -> the byte stream: byte i of a packet goes through branch i mod 12, a FIFO of 17 (i mod 12) cells"""
    fifos = [deque([fill] * (CELLS * j)) for j in range(BRANCHES)]
    out = bytearray()
    for k, b in enumerate(np.asarray(coded, np.uint8).ravel().tolist()):
        f = fifos[k % BRANCHES]
        f.append(b)
        out.append(f.popleft())
    return np.frombuffer(bytes(out), np.uint8).copy()


def to_frames(stream, bitrate_kbps):
    """whole logical frames of 3 * bitrate bytes (what is left over is cut off)"""
    fb = 3 * bitrate_kbps
    n = len(stream) // fb
    return np.ascontiguousarray(stream[:n * fb].reshape(n, fb))


def packets_for(bitrate_kbps, n_frames):
    return -(-3 * bitrate_kbps * n_frames // CODED) + 1


# ---------------------------------------------------------------- receiver
class Receiver:
    def __init__(self, bitrate_kbps):
        self.fb = 3 * bitrate_kbps
        self.pos = 0
        self.run = [0] * CODED
        self.locked, self.start, self.misses = False, 0, 0
        self.fifos, self.row, self.lock_starts, self.lock_emitted = None, [], 0, 0
        self.last = {}                     # pid -> counter of its last good packet
        self.census = []                   # [pid, packets, discontinuities, duplicates, scrambled], in order of appearance
        self.pids_overflowed = 0

    def _deinterleave(self, q, b, done):
        """byte y[q] of the lock into branch (q - start) mod 12, a FIFO of 17 (11 - j) cells; what comes out is byte
        q - start - 2244 of the lock's coded stream"""
        j = (q - self.start) % BRANCHES
        f = self.fifos[j]
        f.append(b)
        o = f.popleft()
        k = q - self.start - CODED * (BRANCHES - 1)
        if k < 0:
            return
        self.row.append(o)
        if len(self.row) == CODED:
            done.append((self.start + k - (CODED - 1), self.row))
            self.row = []
            self.lock_emitted += 1

    def call(self, frames):
        c = dict.fromkeys(COUNTERS, 0)
        frames = np.asarray(frames, np.uint8)[:, :self.fb] if len(frames) else np.zeros((0, self.fb), np.uint8)
        c["cifs"], c["bytes"] = len(frames), len(frames) * self.fb
        done = []
        for b in frames.ravel().tolist():
            q, phi = self.pos, self.pos % CODED
            hit = b == SYNC
            self.run[phi] = min(self.run[phi] + 1, 255) if hit else 0
            if not self.locked:
                if self.run[phi] >= LOCK_RUN:
                    self.locked, self.start, self.misses = True, q, 0
                    self.fifos = [deque([None] * (CELLS * (BRANCHES - 1 - j))) for j in range(BRANCHES)]
                    self.row, self.lock_starts, self.lock_emitted = [], 0, 0
                    c["locks"] += 1
                    c["sync_hits"] += 1
            elif phi == self.start % CODED:
                if hit:
                    self.misses = 0
                    c["sync_hits"] += 1
                else:
                    self.misses += 1
                    if self.misses == LOSS_MISSES:
                        self.locked = False
                        c["lock_losses"] += 1
                        c["packets_dropped"] += self.lock_starts - self.lock_emitted
            if self.locked:
                if phi == self.start % CODED:
                    self.lock_starts += 1
                self._deinterleave(q, b, done)
            self.pos += 1
        ts = np.zeros((len(done), TS), np.uint8)
        rec = np.zeros(len(done), RECORD_DTYPE)
        if done:
            rows = np.array([r for _, r in done], np.uint8)
            fixed, verdicts = F.correct_rows(rows)
            for i, ((s, _), v) in enumerate(zip(done, verdicts)):
                x = fixed[i].copy()
                r = rec[i]
                r["position"] = s & 0xFFFFFFFF
                if v < 0:
                    r["status"] = 2
                    x[1] |= 0x80
                    c["packets_uncorrectable"] += 1
                elif v > 0:
                    differ = np.nonzero(fixed[i] != rows[i])[0]
                    r["status"] = 1
                    r["corrected_data"], r["corrected_parity"] = int((differ < TS).sum()), int((differ >= TS).sum())
                    c["packets_corrected"] += 1
                    c["bytes_corrected"] += int(r["corrected_data"])
                    c["parity_bytes_corrected"] += int(r["corrected_parity"])
                else:
                    c["packets_clean"] += 1
                ts[i] = x[:TS]
                pid, b3 = ((int(x[1]) & 0x1F) << 8) | int(x[2]), int(x[3])
                r["pid"], r["byte3"] = pid, b3
                exempt = bool(b3 & 0x20) and x[4] >= 1 and bool(x[5] & 0x80)
                r["flags"] = 1 if exempt else 0
                if v < 0:
                    continue
                cc, verdict = b3 & 15, ""
                prev = self.last.get(pid)
                if prev is None:
                    if len(self.census) < 32:
                        self.census.append([pid, 0, 0, 0, 0])
                    else:
                        self.pids_overflowed += 1
                elif pid != NULL_PID and not exempt:
                    if b3 & 0x10:
                        verdict = "" if cc == (prev + 1) & 15 else "duplicates" if cc == prev else "discontinuities"
                    else:
                        verdict = "" if cc == prev else "discontinuities"
                if verdict:
                    c[verdict] += 1
                for e in self.census:
                    if e[0] == pid:
                        e[1] += 1
                        e[2] += verdict == "discontinuities"
                        e[3] += verdict == "duplicates"
                        e[4] += (b3 & 0xC0) != 0
                self.last[pid] = cc
        c["packets_emitted"] = len(done)
        c["locked"], c["phase"] = int(self.locked), self.start % CODED if self.locked else -1
        c["pids"], c["pids_overflowed"] = len(self.census), self.pids_overflowed
        return ts, rec, c
