#!/usr/bin/env python3
"""Time dabgpu_dmb_follow_dev on 64 ensembles with one 544 kbit/s T-DMB sub-channel each, beside dabgpu_packet_fec_dev on
the same number of bytes and against the host twin (GPU box).

  python tools/dmb_time.py [--streams 64] [--frames 16,256] [--rounds 10] [--no-host] [--out profiles/dmb_time.txt] [--limit 900]

One visit to the GPU, in a child process that is ended after --limit seconds.  Every entry carries the same transport stream
(random payload on five PIDs, RS(204,188), the 12-branch interleaver) from a different frame on, in two conditions: clean, and
with a burst of 96 consecutive bytes once per logical frame (8 errors in each of 12 packets, the bound; a frame holds 8 packets,
so the bursts of neighbouring frames meet in 4 of every 8 packets, which then lie beyond it).  Per batch shape and condition, after two warm-up rounds, --rounds interleaved rounds of
  (a) the DMB call, the state records swapped between calls
  (b) dabgpu_packet_fec_dev on as many bytes: streams * 17 / 16 entries of 512 kbit/s (the largest it takes) of random bytes --
      it finds no FEC frame, so it moves and scans but corrects nothing: a floor for a call that reads and writes these bytes
each timed between two events on the stream; the median and the spread of the rounds are printed.  Every round replays the
same frames behind the state of the round before, so the 11 packets that straddle the seam are uncorrectable in every call
(11 per entry in the clean condition's counts).  Then (c) the host twin
dabgpu_dmb_follow_host on the same table in host memory (wall time, one thread, one call)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "sdrplusplus-dab-radio-plugin_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

KBPS, FB = 544, 3 * 544


def gf_tables(np):
    exp, log, x = np.zeros(512, np.int64), np.zeros(256, np.int64), 1
    for i in range(255):
        exp[i], log[x] = x, i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    exp[255:510] = exp[:255]
    return exp, log


def transport_stream(np, n_bytes, seed):
    """the interleaved byte stream of n_bytes: packets of five PIDs with counters in order, systematic RS(204,188) (generator
    prod (x + alpha^i), i = 0..15, by LFSR division on all packets at once), byte i of a packet delayed by 204 (i mod 12)"""
    rng = np.random.default_rng(seed)
    n = n_bytes // 204 + 13
    exp, log = gf_tables(np)
    mul = lambda a, b: np.where((a == 0) | (b == 0), 0, exp[log[a] + log[b]])
    g = np.array([1], np.int64)
    for i in range(16):                                        # g[k]: the coefficient of x^k
        g = np.concatenate([[0], g]) ^ np.concatenate([mul(g, np.full(g.size, exp[i])), [0]])
    pk = rng.integers(0, 256, (n, 188), dtype=np.int64)
    pk[pk == 0x47] = 0x46
    pids = np.array([0x000, 0x100, 0x111, 0x112, 0x113])[rng.integers(0, 5, n)]
    cc = np.zeros(n, np.int64)
    for p in np.unique(pids):
        cc[pids == p] = np.arange((pids == p).sum()) & 15
    pk[:, 0], pk[:, 1], pk[:, 2], pk[:, 3] = 0x47, pids >> 8, pids & 0xFF, 0x10 | cc
    reg = np.zeros((n, 16), np.int64)
    gh = g[:16][::-1]
    for c in range(188):
        fb = reg[:, 0] ^ pk[:, c]
        reg = np.concatenate([reg[:, 1:], np.zeros((n, 1), np.int64)], axis=1) ^ mul(fb[:, None], gh[None, :])
    coded = np.concatenate([pk, reg], axis=1).astype(np.uint8)
    y = np.zeros(n * 204 + 2244, np.uint8)
    i = np.arange(204)
    at = (np.arange(n) * 204)[:, None] + (204 * (i % 12) + i)[None, :]
    y[at] = coded
    return y[:n_bytes]


def child(a):
    import numpy as np
    import torch
    import dabgpu
    dev = torch.device("cuda", 0)
    lines = ["dmb_time: %d ensembles, one %d kbit/s T-DMB sub-channel each, %s" % (a.streams, KBPS, torch.cuda.get_device_name(0))]
    sb = dabgpu.dmb_state_bytes()
    n_fec = a.streams * 17 // 16
    with dabgpu.Context(device=0, max_frames=64) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)

        def between_events(run):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run()
            e1.record(stream)
            ctx.sync()
            return e0.elapsed_time(e1)

        for fps in a.frames:
            n_cifs = 4 * fps
            m = dabgpu.dmb_max_packets(KBPS, n_cifs)
            base = transport_stream(np, (n_cifs + a.streams) * FB, 7)
            for label, burst in (("clean", False), ("a 96-byte burst in every logical frame", True)):
                keep, swap, hswap, results = [], [[], []], [[], []], []
                for e in range(a.streams):
                    host = base[e * FB:(e + n_cifs) * FB].reshape(n_cifs, FB).copy()
                    if burst:
                        rng = np.random.default_rng(e)
                        host[:, 500:596] ^= rng.integers(1, 256, (n_cifs, 96), dtype=np.uint8)
                    frames = torch.from_numpy(host).to(dev)
                    z = lambda n: torch.zeros((n,), dtype=torch.uint8, device=dev)
                    ts, rec, s0, s1, res = z((m * 188 + 15) // 16 * 16), z(m * 16), z(sb), z(sb), z(80)
                    h = [np.zeros(m * 188 + 16, np.uint8), np.zeros(m * 16 + 16, np.uint8), np.zeros(sb + 16, np.uint8), np.zeros(sb + 16, np.uint8), np.zeros(80, np.uint8)]
                    al = [x[-x.ctypes.data % 16:] for x in h[:4]]
                    keep += [frames, ts, rec, s0, s1, host, h]
                    results.append(res)
                    for side, (si, so) in enumerate(((s0, s1), (s1, s0))):
                        swap[side].append(dabgpu.DmbEntry(frames.data_ptr(), FB, KBPS, m, ts.data_ptr(), rec.data_ptr(), si.data_ptr(), so.data_ptr(), res.data_ptr()))
                        hswap[side].append(dabgpu.DmbEntry(host.ctypes.data, FB, KBPS, m, al[0].ctypes.data, al[1].ctypes.data, al[2 + side].ctypes.data,
                                                           al[3 - side].ctypes.data, h[4].ctypes.data))
                fswap = [[], []]
                for e in range(n_fec):
                    fbs = dabgpu.packet_fec_state_bytes(512)
                    fin = torch.randint(0, 256, (n_cifs, 1536), dtype=torch.uint8, device=dev)
                    fout = torch.zeros((n_cifs, 1536), dtype=torch.uint8, device=dev)
                    f0, f1, fc = (torch.zeros((n,), dtype=torch.uint8, device=dev) for n in (fbs, fbs, 48))
                    keep += [fin, fout, f0, f1, fc]
                    for side, (si, so) in enumerate(((f0, f1), (f1, f0))):
                        fswap[side].append(dabgpu.PacketFecEntry(fin.data_ptr(), 1536, 512, 0, fout.data_ptr(), 1536, si.data_ptr(), so.data_ptr(), fc.data_ptr()))
                torch.cuda.synchronize()
                turn = [0, 0]

                def dmb():
                    ctx.dmb_follow_dev(swap[turn[0]], n_cifs)
                    turn[0] ^= 1

                def fec():
                    ctx.packet_fec_dev(fswap[turn[1]], n_cifs)
                    turn[1] ^= 1

                ta, tb = [], []
                for r in range(a.rounds + 2):
                    x, y = between_events(dmb), between_events(fec)
                    if r >= 2:
                        ta.append(x)
                        tb.append(y)
                rc = np.stack([c.cpu().numpy().view(dabgpu.DMB_RESULT_DTYPE)[0] for c in results])
                lines += ["%d x %d frames, %s (%d logical frames, %d bytes per entry; the last DMB call: %d packets emitted, %d clean, %d corrected, %d "
                          "uncorrectable, %d bytes corrected, %d discontinuities, %d of %d entries locked):"
                          % (a.streams, fps, label, n_cifs, n_cifs * FB, rc["packets_emitted"].sum(), rc["packets_clean"].sum(), rc["packets_corrected"].sum(),
                             rc["packets_uncorrectable"].sum(), rc["bytes_corrected"].sum() + rc["parity_bytes_corrected"].sum(), rc["discontinuities"].sum(),
                             rc["locked"].sum(), a.streams),
                          "  (a) the DMB call                              %9.3f ms between events (median of %d interleaved rounds, %.3f .. %.3f)"
                          % (float(np.median(ta)), a.rounds, min(ta), max(ta)),
                          "  (b) dabgpu_packet_fec_dev, %3d x 512 kbit/s    %9.3f ms between events (median of %d interleaved rounds, %.3f .. %.3f)"
                          % (n_fec, float(np.median(tb)), a.rounds, min(tb), max(tb))]
                if not a.no_host:
                    t0 = time.perf_counter()
                    dabgpu.dmb_follow_host(hswap[0], n_cifs)
                    wall = (time.perf_counter() - t0) * 1e3
                    lines += ["  (c) the host twin of (a), same table          %9.3f ms wall, one thread, one call         (c) / (a) = %.1f" % (wall, wall / float(np.median(ta)))]
                del keep, swap, hswap, fswap, results
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", default="16,256", help="frames per stream, one batch shape each")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmb_time.txt"))
    ap.add_argument("--limit", type=int, default=900, help="seconds the GPU visit may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        a.frames = [int(x) for x in a.frames.split(",")]
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--streams", str(a.streams), "--frames", a.frames, "--rounds", str(a.rounds),
           "--out", a.out] + (["--no-host"] if a.no_host else [])
    try:
        sys.exit(subprocess.run(cmd, timeout=a.limit).returncode)
    except subprocess.TimeoutExpired:
        sys.exit("dmb_time: the GPU visit took more than %d s and was ended" % a.limit)


if __name__ == "__main__":
    main()
