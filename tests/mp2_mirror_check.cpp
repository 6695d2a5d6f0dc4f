// mp2_mirror_check.cpp -- the host mirror's layer-II channel on its own (tests/test_mp2_mirror.py builds and runs this; it
// links nothing of libdabgpu: Basic_DAB_Channel is header-only and reads PAD through include/dabgpu_mp2_frame.h and the
// two walks).  argv: bit rate, file of logical frames -> one line of counters, the label in hex, one line per slide.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "basic_radio/basic_dab_channel.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int bitrate = std::atoi(argv[1]);
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    Subchannel sub{};
    Basic_DAB_Channel channel(sub, bitrate);
    int new_slides = 0;
    channel.GetSlideshowManager().OnNewSlideshow().Attach([&new_slides](std::shared_ptr<Basic_Slideshow> &) { new_slides++; });
    std::vector<uint8_t> lf(size_t(bitrate) * 3);
    while (std::fread(lf.data(), 1, lf.size(), f) == lf.size()) channel.Process(lf);
    std::fclose(f);
    const auto &params = channel.GetAudioParams();
    std::printf("frames=%d header_errors=%d is_error=%d rate=%u kbps=%u stereo=%d checked=%d crc_errors=%d no_crc=%d charset=%d new_slides=%d\n",
                channel.GetTotalFrames(), channel.GetTotalHeaderErrors(), int(channel.GetIsError()), params ? params->sample_rate : 0u,
                params ? params->bitrate_kbps : 0u, params ? int(params->is_stereo) : -1, channel.GetTotalCheckedFrames(),
                channel.GetTotalCrcErrors(), channel.GetTotalFramesWithoutCrc(), channel.GetDynamicLabelCharset(), new_slides);
    std::printf("label=");
    for (unsigned char v : channel.GetDynamicLabel()) std::printf("%02x", v);
    std::printf("\n");
    for (auto &s : channel.GetSlideshowManager().GetSlideshows()) {
        std::printf("slide id=%u name=%s bytes=%zu image=", unsigned(s->transport_id), s->name.c_str(), s->image_data.size());
        for (uint8_t v : s->image_data) std::printf("%02x", v);
        std::printf("\n");
    }
    return 0;
}
