// dmb_mirror_check.cpp -- the host mirror's Basic_DMB_Channel on its own (tests/test_dmb_mirror.py builds this under
// AddressSanitizer and UBSan and runs it; the channel runs include/dabgpu_dmb.h directly, so nothing of libdabgpu and nothing
// of the test-only fake ABI is linked):
//   dmb_mirror_check bitrate frames_file ts_file
// feeds the file's logical frames of 3 * bitrate bytes to Process one by one, writes every packet OnTransportPackets hands out
// to ts_file and prints the channel's statistics and census: what dabgpu_dmb_follow_host gives for the frames in one call.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "basic_radio/basic_dmb_channel.h"

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const int kbps = std::atoi(argv[1]);
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<uint8_t> bytes;
    for (uint8_t buf[4096]; size_t n = std::fread(buf, 1, sizeof buf, f);) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    std::FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 2;

    Subchannel sub{};
    Basic_DMB_Channel channel(sub, kbps);
    int packets = 0, handed = 0;
    channel.OnTransportPackets().Attach([&](tcb::span<const uint8_t> ts, tcb::span<const dabgpu_dmb::Record> records) {
        if (ts.size() != records.size() * 188) std::exit(3);
        std::fwrite(ts.data(), 1, ts.size(), out);
        packets += int(records.size());
        handed++;
    });
    const size_t fb = size_t(3 * kbps);
    for (size_t at = 0; at + fb <= bytes.size(); at += fb) channel.Process(tcb::span<const uint8_t>(bytes.data() + at, fb));
    channel.Process(tcb::span<const uint8_t>(bytes.data(), bytes.size() < 5 ? bytes.size() : 5));      // a frame of another size: ignored
    std::fclose(out);
    const dabgpu_dmb::Result &r = channel.GetStatistics();
    std::printf("cifs=%d bytes=%d sync_hits=%d locks=%d lock_losses=%d emitted=%d clean=%d corrected=%d uncorrectable=%d dropped=%d "
                "bytes_corrected=%d parity_bytes_corrected=%d discontinuities=%d duplicates=%d locked=%d phase=%d pids=%d pids_overflowed=%d "
                "packets_deferred=%d packets_lost=%d\n",
                r.cifs, r.bytes, r.sync_hits, r.locks, r.lock_losses, r.packets_emitted, r.packets_clean, r.packets_corrected, r.packets_uncorrectable,
                r.packets_dropped, r.bytes_corrected, r.parity_bytes_corrected, r.discontinuities, r.duplicates, r.locked, r.phase, r.pids,
                r.pids_overflowed, r.packets_deferred, r.packets_lost);
    std::printf("handed=%d ignored=%d\n", packets, channel.GetTotalFramesIgnored());
    for (const auto &c : channel.GetCensus())
        std::printf("pid=%u packets=%u discontinuities=%u duplicates=%u scrambled=%u\n", unsigned(c.pid), c.packets, c.discontinuities, c.duplicates,
                    c.scrambled);
    return handed > 0 ? 0 : 4;
}
