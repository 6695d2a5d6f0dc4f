// packet_groups_mirror_check.cpp -- the host mirror's data packet channel and FIC database on their own, their data-group side
// (tests/test_packet_groups_mirror.py builds and runs this; it links nothing of libdabgpu: Basic_Data_Packet_Channel is
// header-only and runs include/dabgpu_data_groups.h).
//   channel <bit rate> <FEC scheme> <file of logical frames> <address:mode:keep> ...
//       -> one line per data group as OnDataGroup hands it out (record fields, bytes in hex), one line per OnRawData call (its break records as offset/length/cif/slot/flags),
//          then one line of counters per address
//   fic <file of FIBs, 32 bytes each>
//       -> one line per user application of the database, and per packet component the types joined to it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "basic_radio/basic_data_packet_channel.h"
#include "dab/fic/fic_parser.h"

static void hex(const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) std::printf("%02x", p[i]);
}

static int channel_main(int argc, char **argv) {
    if (argc < 6) return 2;
    const int bitrate = std::atoi(argv[2]), fec = std::atoi(argv[3]);
    std::FILE *f = std::fopen(argv[4], "rb");
    if (!f) return 2;
    Subchannel sub{};
    Basic_Data_Packet_Channel channel(sub, fec);
    int refused = 0;
    for (int i = 5; i < argc; i++) {
        int address = 0, mode = 0, keep = 0;
        if (std::sscanf(argv[i], "%d:%d:%d", &address, &mode, &keep) != 3) return 2;
        refused += !channel.FollowDataGroups(address, mode, keep != 0);
    }
    channel.OnDataGroup().Attach([](int address, const dabgpu_groups::Record &r, tcb::span<const uint8_t> g) {
        std::printf("group address=%d offset=%d length=%d cif=%d slot=%d type=%d continuity=%d repetition=%d flags=%d extension=%d segment=%d "
                    "transport_id=%d data_offset=%d data_length=%d bytes=",
                    address, r.offset, r.length, r.cif, r.slot, r.type, r.continuity, r.repetition, r.flags, r.extension, r.segment, r.transport_id,
                    r.data_offset, r.data_length);
        hex(g.data(), g.size());
        std::printf("\n");
    });
    channel.OnRawData().Attach([](int address, tcb::span<const uint8_t> bytes, tcb::span<const dabgpu_groups::Record> breaks) {
        std::printf("raw address=%d breaks=%zu at=", address, breaks.size());
        for (const auto &r : breaks) std::printf("%d/%d/%d/%d/%d,", r.offset, r.length, r.cif, r.slot, r.flags);
        std::printf(" bytes=");
        hex(bytes.data(), bytes.size());
        std::printf("\n");
    });
    std::vector<uint8_t> lf(size_t(bitrate) * 3);
    while (std::fread(lf.data(), 1, lf.size(), f) == lf.size()) channel.Process(lf);
    std::fclose(f);
    std::printf("frames=%d ignored=%d addresses=%d refused=%d\n", channel.GetTotalFrames(), channel.GetTotalFramesIgnored(),
                channel.GetTotalDataAddresses(), refused);
    static const char *names[] = {"cifs", "slots", "slots_bad", "packets_fec", "packets_padding", "packets_other", "packets_followed", "continuity_breaks",
                                  "packets_malformed", "packets_command", "packets_orphan", "groups_opened", "groups_unfinished", "groups_too_long",
                                  "group_bytes", "groups_closed", "groups_malformed", "groups_crc_failed", "groups_no_crc", "groups_repeated",
                                  "groups_emitted", "groups_no_room", "bytes_emitted", "bytes_no_room"};
    for (int a = 0; a < channel.GetTotalDataAddresses(); a++) {
        const int32_t *v = reinterpret_cast<const int32_t *>(&channel.GetDataGroupCounters(a));
        std::printf("counters address=%d mode=%d", channel.GetDataAddress(a), channel.GetDataMode(a));
        for (size_t i = 0; i < sizeof names / sizeof *names; i++) std::printf(" %s=%d", names[i], v[i]);
        std::printf("\n");
    }
    return 0;
}

static int fic_main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    DAB_Database db;
    DAB_Database_Updater updater(db);
    FIC_Parser parser(updater);
    uint8_t fib[32];
    while (std::fread(fib, 1, sizeof fib, f) == sizeof fib) parser.ProcessFIB(tcb::span<const uint8_t>(fib, sizeof fib));
    std::fclose(f);
    for (const auto &u : db.user_applications) {
        std::printf("application sid=%u scids=%d type=%d data=", unsigned(u.service_id), u.scids, u.type);
        hex(u.data.data(), u.data.size());
        std::printf("\n");
    }
    for (const auto &pc : db.packet_components) {
        std::printf("component scid=%d subchid=%d address=%d types=", pc.scid, pc.is_described ? int(pc.subchannel_id) : -1,
                    pc.is_described ? int(pc.packet_address) : -1);
        for (const UserApplication *u : db.UserApplicationsOf(pc)) std::printf("%d,", u->type);
        std::printf("\n");
    }
    for (const auto &s : db.subchannels) {
        std::printf("subchannel id=%d types=", int(s.id));
        for (const UserApplication *u : db.UserApplicationsOfSubchannel(s.id)) std::printf("%d,", u->type);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "channel")) return channel_main(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "fic")) return fic_main(argc, argv);
    return 2;
}
