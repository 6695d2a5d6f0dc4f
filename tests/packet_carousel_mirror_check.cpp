// packet_carousel_mirror_check.cpp -- the host mirror's data packet channel on its own, its directory-mode side
// (tests/test_packet_carousel_mirror.py builds and runs this; it links nothing of libdabgpu: Basic_Data_Packet_Channel is
// header-only and runs include/dabgpu_packet_walk.h and include/dabgpu_mot_carousel.h).
// argv: bit rate, FEC scheme, file of logical frames, packet addresses ... -> the lines of packet_mirror_check.cpp (channel,
// one per address, one per slide), then per address one line of carousel counters, one line for its current directory (hex)
// and one line per object delivered (header and body in hex).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "basic_radio/basic_data_packet_channel.h"

static void hex(const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) std::printf("%02x", p[i]);
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const int bitrate = std::atoi(argv[1]), fec = std::atoi(argv[2]);
    std::FILE *f = std::fopen(argv[3], "rb");
    if (!f) return 2;
    Subchannel sub{};
    Basic_Data_Packet_Channel channel(sub, fec);
    int refused = 0;
    for (int i = 4; i < argc; i++) refused += !channel.FollowAddress(std::atoi(argv[i]));
    int new_slides = 0;
    channel.GetSlideshowManager().OnNewSlideshow().Attach([&new_slides](std::shared_ptr<Basic_Slideshow> &) { new_slides++; });
    std::vector<uint8_t> lf(size_t(bitrate) * 3);
    while (std::fread(lf.data(), 1, lf.size(), f) == lf.size()) channel.Process(lf);
    std::fclose(f);
    std::printf("frames=%d ignored=%d addresses=%d refused=%d new_slides=%d\n", channel.GetTotalFrames(), channel.GetTotalFramesIgnored(),
                channel.GetTotalAddresses(), refused, new_slides);
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
        hex(s->image_data.data(), s->image_data.size());
        std::printf("\n");
    }
    for (int a = 0; a < channel.GetTotalAddresses(); a++) {
        const auto &c = channel.GetCarouselCounters(a);
        const auto &h = c.head;
        std::printf("carousel address=%d packets_followed=%d continuity_breaks=%d groups_opened=%d group_bytes=%d groups_ok=%d groups_crc_failed=%d "
                    "groups_ignored_type=%d groups_malformed=%d groups_repeated=%d segments_placed=%d segments_early_last=%d objects_completed=%d "
                    "objects_mismatched=%d objects_too_large=%d groups_header_mode=%d groups_compressed_directory=%d groups_unlisted=%d "
                    "directories_completed=%d directories_mismatched=%d directories_too_large=%d objects_stale=%d objects_evicted=%d "
                    "objects_dropped=%d objects_deferred=%d directory_id=%d directory_bytes=%d directory_objects=%d directory_period=%d\n",
                    channel.GetAddress(a), h.packets_followed, h.continuity_breaks, h.groups_opened, h.group_bytes, h.mot.groups_ok, h.mot.groups_crc_failed,
                    h.mot.groups_ignored_type, h.mot.groups_malformed, h.mot.groups_repeated, h.mot.segments_placed, h.mot.segments_early_last,
                    h.mot.objects_completed, h.mot.objects_mismatched, h.mot.objects_too_large, c.groups_header_mode, c.groups_compressed_directory,
                    c.groups_unlisted, c.directories_completed, c.directories_mismatched, c.directories_too_large, c.objects_stale, c.objects_evicted,
                    c.objects_dropped, c.objects_deferred, c.directory_id, c.directory_bytes, c.directory_objects, c.directory_period);
        const auto d = channel.GetDirectory(a);
        std::printf("directory address=%d bytes=%zu data=", channel.GetAddress(a), d.size());
        hex(d.data(), d.size());
        std::printf("\n");
        for (const auto &o : channel.GetCarouselObjects(a)) {
            std::printf("object address=%d id=%d type=%d subtype=%d directory=%d header=", channel.GetAddress(a), o.entry.transport_id, o.entry.content_type,
                        o.entry.content_subtype, o.directory_id);
            hex(o.header.data(), o.header.size());
            std::printf(" body=");
            hex(o.body.data(), o.body.size());
            std::printf("\n");
        }
    }
    return 0;
}
