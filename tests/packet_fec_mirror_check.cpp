// packet_fec_mirror_check.cpp -- the host mirror's data packet channel on an FEC-protected sub-channel, on its own
// (tests/test_packet_fec_mirror.py builds and runs this; it links nothing of libdabgpu: Basic_Data_Packet_Channel is
// header-only and runs include/dabgpu_packet_fec.h in front of include/dabgpu_packet_walk.h).  The correction is switched as
// BasicRadio switches it: on when the FEC scheme is 1.
// argv: bit rate, FEC scheme, file of logical frames, packet addresses ... -> one line of channel counters, one line of the
// FEC counters, one line of counters per address, one line per slide (name and image in hex).
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
    int refused = 0;
    for (int i = 4; i < argc; i++) refused += !channel.FollowAddress(std::atoi(argv[i]));
    int new_slides = 0;
    channel.GetSlideshowManager().OnNewSlideshow().Attach([&new_slides](std::shared_ptr<Basic_Slideshow> &) { new_slides++; });
    std::vector<uint8_t> lf(size_t(bitrate) * 3);
    while (std::fread(lf.data(), 1, lf.size(), f) == lf.size()) channel.Process(lf);
    std::fclose(f);
    std::printf("frames=%d ignored=%d addresses=%d refused=%d new_slides=%d\n", channel.GetTotalFrames(), channel.GetTotalFramesIgnored(),
                channel.GetTotalAddresses(), refused, new_slides);
    const auto &q = channel.GetFecCounters();
    std::printf("corrects=%d cifs=%d slots=%d marks=%d frames=%d frames_cut=%d frames_overlapping=%d rows_clean=%d rows_corrected=%d rows_uncorrectable=%d "
                "bytes_corrected=%d parity_bytes_corrected=%d\n", int(channel.GetFecCorrection()), q.cifs, q.slots, q.marks, q.frames, q.frames_cut,
                q.frames_overlapping, q.rows_clean, q.rows_corrected, q.rows_uncorrectable, q.bytes_corrected, q.parity_bytes_corrected);
    for (int a = 0; a < channel.GetTotalAddresses(); a++) {
        const auto &c = channel.GetCounters(a);
        std::printf("address=%d cifs=%d slots=%d slots_bad=%d packets_fec=%d packets_padding=%d packets_other=%d packets_followed=%d continuity_breaks=%d "
                    "packets_malformed=%d packets_command=%d packets_orphan=%d groups_opened=%d groups_unfinished=%d groups_too_long=%d group_bytes=%d "
                    "groups_ok=%d groups_crc_failed=%d groups_ignored_type=%d groups_malformed=%d groups_repeated=%d objects_completed=%d\n",
                    channel.GetAddress(a), c.cifs, c.slots, c.slots_bad, c.packets_fec, c.packets_padding, c.packets_other, c.packets_followed,
                    c.continuity_breaks, c.packets_malformed, c.packets_command, c.packets_orphan, c.groups_opened, c.groups_unfinished,
                    c.groups_too_long, c.group_bytes, c.mot.groups_ok, c.mot.groups_crc_failed, c.mot.groups_ignored_type, c.mot.groups_malformed,
                    c.mot.groups_repeated, c.mot.objects_completed);
    }
    for (auto &s : channel.GetSlideshowManager().GetSlideshows()) {
        std::printf("slide id=%u name=", unsigned(s->transport_id));
        for (unsigned char v : s->name) std::printf("%02x", v);
        std::printf(" bytes=%zu image=", s->image_data.size());
        for (uint8_t v : s->image_data) std::printf("%02x", v);
        std::printf("\n");
    }
    return 0;
}
