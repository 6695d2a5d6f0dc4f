// mp2_audio_mirror_check.cpp -- the audio level of the host mirror's layer-II channel on its own (tests/test_mp2_audio_mirror.py
// builds and runs this; it links nothing of libdabgpu: Basic_DAB_Channel is header-only and decodes through
// include/dabgpu_mp2_audio.h).  argv: bit rate, file of logical frames, decode audio (0 / 1), decode data (0 / 1) -> one line
// per logical frame: what GetAudioLevel() says behind it, the floats as their bits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "basic_radio/basic_dab_channel.h"

static unsigned bits_of(float v) {
    unsigned u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const int bitrate = std::atoi(argv[1]);
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    Subchannel sub{};
    Basic_DAB_Channel channel(sub, bitrate);
    channel.GetControls().SetIsDecodeAudio(std::atoi(argv[3]) != 0);
    channel.GetControls().SetIsDecodeData(std::atoi(argv[4]) != 0);
    std::vector<uint8_t> lf(size_t(bitrate) * 3);
    while (std::fread(lf.data(), 1, lf.size(), f) == lf.size()) {
        channel.Process(lf);
        const auto &lv = channel.GetAudioLevel();
        if (!lv) { std::printf("none checked=%d\n", channel.GetTotalCheckedFrames()); continue; }
        std::printf("%d %d %d %d %08x %08x %08x %08x checked=%d\n", int(lv->kind), int(lv->channels), int(lv->cells), int(lv->scf63),
                    bits_of(lv->power[0]), bits_of(lv->power[1]), bits_of(lv->peak[0]), bits_of(lv->peak[1]), channel.GetTotalCheckedFrames());
    }
    std::fclose(f);
    return 0;
}
