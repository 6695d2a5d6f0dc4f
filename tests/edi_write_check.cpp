// edi_write_check.cpp -- dabgpu_edi::write_packet of include/dabgpu_edi.h on its own (tests/test_edi.py builds and runs it and
// holds its output byte for byte to the from-definition writer of tests/edi_reference.py and to the known-answer packet):
//   edi_write_check case.bin > packet.bin
// case.bin: nst (1 byte), the plan's nst STC words (4 bytes each), SEQ (2 bytes, big-endian), dlfc (2), STAT (1), the 96 FIC
// bytes, then every stream's bytes of the CIF in the plan's order.
#include <cstdio>
#include <vector>

#include "dabgpu_edi.h"

namespace ed = dabgpu_edi;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> in;
    for (uint8_t buf[4096]; size_t n = std::fread(buf, 1, sizeof buf, f);) in.insert(in.end(), buf, buf + n);
    std::fclose(f);
    if (in.empty() || in[0] > ed::MAX_STREAMS || in.size() < size_t(1 + 4 * in[0] + 5 + ed::FIC_BYTES)) return 2;
    ed::PlanKey plan{};
    plan.nst = in[0];
    size_t at = 1;
    std::vector<size_t> offset(size_t(plan.nst) + 1, 0);
    for (int k = 0; k < plan.nst; k++) {
        for (int i = 0; i < 4; i++) plan.stc[4 * k + i] = in[at++];
        offset[size_t(k) + 1] = offset[size_t(k)] + 8u * size_t(((plan.stc[4 * k + 2] & 3) << 8) | plan.stc[4 * k + 3]);
    }
    const uint32_t seq = uint32_t(in[at] << 8 | in[at + 1]), dlfc = uint32_t(in[at + 2] << 8 | in[at + 3]), stat = in[at + 4];
    at += 5;
    const uint8_t *fic = in.data() + at, *data = fic + ed::FIC_BYTES;
    if (in.size() != at + size_t(ed::FIC_BYTES) + offset[size_t(plan.nst)]) return 2;
    std::vector<uint8_t> out(size_t(ed::MAX_PACKET), 0);
    const int total = ed::write_packet([&](int i, uint8_t b) { out[size_t(i)] = b; }, plan, seq, dlfc, stat, [&](int i) { return uint32_t(fic[i]); },
                                       [&](int k, int i) { return uint32_t(data[offset[size_t(k)] + size_t(i)]); });
    return std::fwrite(out.data(), 1, size_t(total), stdout) == size_t(total) ? 0 : 1;
}
