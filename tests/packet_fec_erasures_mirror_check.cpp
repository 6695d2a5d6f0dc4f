// packet_fec_erasures_mirror_check.cpp -- the host mirror's data packet channel on an FEC-protected sub-channel with lost
// packets as erasures, on its own (tests/test_packet_fec_erasures_mirror.py builds and runs this; it links nothing of
// libdabgpu: Basic_Data_Packet_Channel is header-only and, with FEC scheme 1, runs include/dabgpu_packet_fec_erasures.h in
// front of include/dabgpu_packet_walk.h).  The correction is switched as BasicRadio switches it: on when the scheme is 1.
// argv: bit rate, FEC scheme, file of logical frames, packet address -> one line of the FEC counters, one line of the
// address's packet counters, one line per slide (image in hex).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "basic_radio/basic_data_packet_channel.h"

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const int bitrate = std::atoi(argv[1]), fec = std::atoi(argv[2]);
    std::FILE *f = std::fopen(argv[3], "rb");
    if (!f) return 2;
    Subchannel sub{};
    Basic_Data_Packet_Channel channel(sub, fec);
    channel.SetFecCorrection(channel.GetFecScheme() == 1);
    if (!channel.FollowAddress(std::atoi(argv[4]))) return 2;
    std::vector<uint8_t> lf(size_t(bitrate) * 3);
    while (std::fread(lf.data(), 1, lf.size(), f) == lf.size()) channel.Process(lf);
    std::fclose(f);
    const auto &q = channel.GetFecErasureCounters();
    const auto &o = channel.GetFecCounters();
    std::printf("corrects=%d same=%d cifs=%d slots=%d marks=%d frames=%d frames_cut=%d frames_overlapping=%d rows_clean=%d rows_corrected=%d "
                "rows_uncorrectable=%d bytes_corrected=%d parity_bytes_corrected=%d slots_suspect=%d frames_with_suspects=%d frames_beyond_erasures=%d "
                "rows_erasure_corrected=%d erased_bytes_changed=%d erasure_other_bytes_corrected=%d\n",
                int(channel.GetFecCorrection()), int(&o == &q.c), q.c.cifs, q.c.slots, q.c.marks, q.c.frames, q.c.frames_cut, q.c.frames_overlapping,
                q.c.rows_clean, q.c.rows_corrected, q.c.rows_uncorrectable, q.c.bytes_corrected, q.c.parity_bytes_corrected, q.slots_suspect,
                q.frames_with_suspects, q.frames_beyond_erasures, q.rows_erasure_corrected, q.erased_bytes_changed, q.erasure_other_bytes_corrected);
    const auto &c = channel.GetCounters(0);
    std::printf("frames=%d slots_bad=%d packets_fec=%d packets_followed=%d continuity_breaks=%d objects_completed=%d\n", channel.GetTotalFrames(), c.slots_bad,
                c.packets_fec, c.packets_followed, c.continuity_breaks, c.mot.objects_completed);
    for (auto &s : channel.GetSlideshowManager().GetSlideshows()) {
        std::printf("slide id=%u bytes=%zu image=", unsigned(s->transport_id), s->image_data.size());
        for (uint8_t v : s->image_data) std::printf("%02x", v);
        std::printf("\n");
    }
    return 0;
}
