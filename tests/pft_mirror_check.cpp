// pft_mirror_check.cpp -- BasicRadio::ProcessPft on its own (tests/test_pft.py builds this with the mirror's sources against
// the TEST-ONLY fake ABI of tests/fake_abi, under AddressSanitizer and UBSan, and runs it):
//   pft_mirror_check pft|edi file piece piece ...
// feeds the file to ProcessPft (a PF fragment stream; the last piece with flush) or to ProcessEdi (the AF packets the
// fragments were made of) in pieces of the given sizes, taken in turn over and over, and prints the read counters, the
// services of the database and one line per channel: the two modes have to print the same from the second line on.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "basic_radio/basic_radio.h"

static void hex(const std::string &s) {
    for (const char v : s) std::printf("%02x", unsigned(uint8_t(v)));
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const bool pft = !std::strcmp(argv[1], "pft");
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<uint8_t> bytes;
    for (uint8_t buf[4096]; size_t n = std::fread(buf, 1, sizeof buf, f);) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    std::vector<size_t> pieces;
    for (int i = 3; i < argc; i++) pieces.push_back(size_t(std::atol(argv[i])));

    BasicRadio radio(get_dab_parameters(1));
    int aus = 0;
    radio.On_Audio_Channel().Attach([&](subchannel_id_t, Basic_Audio_Channel &channel) {
        if (auto *plus = dynamic_cast<Basic_DAB_Plus_Channel *>(&channel)) plus->OnAccessUnit().Attach([&](int, int, tcb::span<const uint8_t>) { aus++; });
    });
    for (size_t at = 0, k = 0; at < bytes.size(); k++) {
        const size_t n = std::min(pieces[k % pieces.size()], bytes.size() - at);
        const tcb::span<const uint8_t> piece(bytes.data() + at, n);
        if (pft) radio.ProcessPft(piece, at + n == bytes.size());
        else radio.ProcessEdi(piece);
        at += n;
    }
    const dabgpu_pft::Head p = radio.GetPftReadTotals();
    std::printf("pft records=%llu packets=%llu lost=%llu recovered=%llu fragments=%llu duplicates=%llu late=%llu missing=%llu skipped=%llu\n",
                (unsigned long long)p.records, (unsigned long long)p.packets, (unsigned long long)p.lost, (unsigned long long)p.recovered,
                (unsigned long long)p.fragments, (unsigned long long)p.duplicates, (unsigned long long)p.late, (unsigned long long)p.missing,
                (unsigned long long)p.skipped);
    auto lock = std::scoped_lock(radio.GetMutex());
    const auto &h = radio.GetEdiReadTotals();
    std::printf("read rows=%llu not_deti=%llu bad_tags=%llu skipped=%llu resyncs=%llu gap_sum=%llu fib_errors=%llu tail=%u fibs=%d\n",
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
            std::printf("packet subchannel=%d frames=%d addresses=%d\n", sc.id, data->GetTotalFrames(), data->GetTotalAddresses());
        } else if (auto *mp2 = dynamic_cast<Basic_DAB_Channel *>(radio.Get_Audio_Channel(sc.id))) {
            std::printf("channel subchannel=%d mp2_frames=%d header_errors=%d crc_errors=%d\n", sc.id, mp2->GetTotalFrames(), mp2->GetTotalHeaderErrors(),
                        mp2->GetTotalCrcErrors());
        } else if (auto *ch = dynamic_cast<Basic_DAB_Plus_Channel *>(radio.Get_Audio_Channel(sc.id))) {
            std::printf("channel subchannel=%d superframes=%d aus=%d handed=%d au_errors=%d label=", sc.id, ch->GetTotalSuperFrames(),
                        ch->GetTotalAccessUnits(), aus, ch->GetTotalAccessUnitErrors());
            hex(std::string(ch->GetDynamicLabel()));
            std::printf("\n");
        }
    }
    return 0;
}
