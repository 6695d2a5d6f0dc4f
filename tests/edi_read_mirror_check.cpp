// edi_read_mirror_check.cpp -- BasicRadio::ProcessEdi on its own (tests/test_edi_read.py builds this with the mirror's
// sources against the TEST-ONLY fake ABI of tests/fake_abi and runs it):
//   edi_read_mirror_check file.edi piece piece ...
// feeds the file to ProcessEdi in pieces of the given sizes, taken in turn over and over, and prints the read counters, the
// services of the database and one line per channel: what the GUI would show.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "basic_radio/basic_radio.h"

static void hex(const std::string &s) {
    for (const char v : s) std::printf("%02x", unsigned(uint8_t(v)));
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> bytes;
    for (uint8_t buf[4096]; size_t n = std::fread(buf, 1, sizeof buf, f);) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    std::vector<size_t> pieces;
    for (int i = 2; i < argc; i++) pieces.push_back(size_t(std::atol(argv[i])));

    BasicRadio radio(get_dab_parameters(1));
    int aus = 0, mp2_frames = 0;
    radio.On_Audio_Channel().Attach([&](subchannel_id_t, Basic_Audio_Channel &channel) {
        if (auto *mp2 = dynamic_cast<Basic_DAB_Channel *>(&channel)) mp2->OnMP2Frame().Attach([&](tcb::span<const uint8_t>) { mp2_frames++; });
        if (auto *plus = dynamic_cast<Basic_DAB_Plus_Channel *>(&channel)) plus->OnAccessUnit().Attach([&](int, int, tcb::span<const uint8_t>) { aus++; });
    });
    size_t calls = 0;
    for (size_t at = 0, k = 0; at < bytes.size(); k++, calls++) {
        const size_t n = std::min(pieces[k % pieces.size()], bytes.size() - at);
        radio.ProcessEdi(tcb::span<const uint8_t>(bytes.data() + at, n));
        at += n;
    }
    auto lock = std::scoped_lock(radio.GetMutex());
    const auto &h = radio.GetEdiReadTotals();
    std::printf("read calls=%zu rows=%llu not_deti=%llu bad_tags=%llu skipped=%llu resyncs=%llu gap_sum=%llu fib_errors=%llu tail=%u fibs=%d\n", calls,
                (unsigned long long)h.rows, (unsigned long long)h.not_deti, (unsigned long long)h.bad_tags, (unsigned long long)h.skipped,
                (unsigned long long)h.resyncs, (unsigned long long)h.gap_sum, (unsigned long long)h.fib_errors, unsigned(h.tail_bytes),
                radio.GetTotalFIBs());
    const auto &db = radio.GetDatabase();
    std::printf("ensemble id=%u label=", unsigned(db.ensemble.id.value));
    hex(db.ensemble.label);
    std::printf("\n");
    for (const auto &sv : db.services) {
        std::printf("service id=%u label=", unsigned(sv.id.value));
        hex(sv.label);
        std::printf("\n");
    }
    auto subs = db.subchannels;
    std::sort(subs.begin(), subs.end(), [](const Subchannel &a, const Subchannel &b) { return a.id < b.id; });
    for (const auto &sc : subs) {
        if (auto *data = radio.Get_Data_Packet_Channel(sc.id)) {
            std::printf("packet subchannel=%d frames=%d addresses=%d followed=%d objects=%d\n", sc.id, data->GetTotalFrames(), data->GetTotalAddresses(),
                        data->GetTotalAddresses() ? data->GetCounters(0).packets_followed : 0,
                        data->GetTotalAddresses() ? data->GetCounters(0).mot.objects_completed : 0);
        } else if (auto *mp2 = dynamic_cast<Basic_DAB_Channel *>(radio.Get_Audio_Channel(sc.id))) {
            std::printf("channel subchannel=%d mp2_frames=%d handed=%d header_errors=%d crc_errors=%d label=", sc.id, mp2->GetTotalFrames(), mp2_frames,
                        mp2->GetTotalHeaderErrors(), mp2->GetTotalCrcErrors());
            hex(std::string(mp2->GetDynamicLabel()));
            std::printf("\n");
        } else if (auto *ch = dynamic_cast<Basic_DAB_Plus_Channel *>(radio.Get_Audio_Channel(sc.id))) {
            std::printf("channel subchannel=%d superframes=%d aus=%d handed=%d au_errors=%d label=", sc.id, ch->GetTotalSuperFrames(),
                        ch->GetTotalAccessUnits(), aus, ch->GetTotalAccessUnitErrors());
            hex(std::string(ch->GetDynamicLabel()));
            std::printf("\n");
        }
    }
    return 0;
}
