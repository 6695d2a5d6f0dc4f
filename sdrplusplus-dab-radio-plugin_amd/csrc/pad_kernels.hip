// pad_kernels.hip -- dynamic labels from the PAD of DAB+ access units (dabgpu_pad_labels_dev; contract: include/dabgpu.h,
// the walk itself: include/dabgpu_pad_walk.h, shared with the host twin and the host mirror).
//
// One wave64 per followed sub-channel.  The state record comes into LDS with 16-byte accesses and goes back the same
// way.  Per super-frame the wave makes three rounds of memory latency, whatever the number of access units: the status
// row (fetched a super-frame ahead); the three bytes in front of every access unit (the data stream element's tag and count); the PAD bytes of all of
// them.  Lane 0 then runs the walk over what lies in LDS -- the walk is a byte-serial state machine (a data group's
// length is known from its prefix, a segment completes a label), so there is nothing for the other lanes to do but fetch.
#include <hip/hip_runtime.h>

#include "../../include/dabgpu_pad_walk.h"
#include "kernels.hpp"

namespace dabk {
namespace {

namespace pad = dabgpu_pad;

constexpr int PAD_MAX_AUS = 7;          // au_start[8] names at most seven
constexpr int PAD_AU_BYTES = 528;       // tag, count, escape count and at most 255 + 255 PAD bytes, rounded up to 16

static_assert(sizeof(pad::State) % 16 == 0 && sizeof(pad::Label) % 4 == 0 && sizeof(pad::Counters) % 4 == 0, "copied by words");
static_assert(sizeof(SuperframeStatus) == 64 && sizeof(FollowResult) == 32, "records of the follow call");

__global__ __launch_bounds__(64) void pad_labels_kernel(const PadEntry *table) {
    __shared__ pad::State st;
    __shared__ pad::Counters c;
    __shared__ int32_t row[16];
    __shared__ int32_t au_len[8], au_begin[8];
    __shared__ __attribute__((aligned(16))) uint8_t bytes[PAD_MAX_AUS][PAD_AU_BYTES];
    const PadEntry e = table[blockIdx.x];
    const int lane = threadIdx.x, s = e.s;
    constexpr int STATE_WORDS = int(sizeof(pad::State) / 16);
    if (lane < STATE_WORDS)
        reinterpret_cast<uint4 *>(&st)[lane] = e.state_in ? reinterpret_cast<const uint4 *>(e.state_in)[lane] : make_uint4(0u, 0u, 0u, 0u);
    int n_sf = reinterpret_cast<const FollowResult *>(e.follow)->n_superframes;
    n_sf = n_sf < 0 ? 0 : n_sf > e.max_superframes ? e.max_superframes : n_sf;
    if (lane < int(sizeof(pad::Counters) / 4)) reinterpret_cast<int32_t *>(&c)[lane] = 0;
    __syncthreads();
    if (lane == 0) pad::sanitize(st);
    // the status row of super-frame k + 1 is on its way while super-frame k is walked
    const int32_t *status = reinterpret_cast<const int32_t *>(e.status);
    int32_t next_word = lane < 16 && n_sf > 0 ? status[lane] : 0;
    for (int k = 0; k < n_sf; k++) {
        __syncthreads();                                               // (the walk of the super-frame before has read `bytes`)
        if (lane < 16) {
            row[lane] = next_word;
            if (k + 1 < n_sf) next_word = status[16 * size_t(k + 1) + lane];
        }
        __syncthreads();
        const uint8_t *data = reinterpret_cast<const uint8_t *>(e.data) + size_t(k) * e.data_stride;
        const int n_aus = pad::visited_aus(row[0], row[3]);
        {   // lanes 8 a .. 8 a + 2: the first three bytes of access unit a
            const int a = lane >> 3, j = lane & 7;
            if (a < n_aus) {
                int b = 0;
                const int len = pad::au_span(row[0], row[3], row[4], row[5 + a], row[6 + a], a, s, &b);
                if (j == 7) { au_len[a] = len; au_begin[a] = b; }
                if (j < 3 && j < len) bytes[a][j] = data[b + j];
            }
        }
        __syncthreads();
        for (int a = 0; a < n_aus; a++) {
            const int len = au_len[a];
            // what the walk may read: nothing of an access unit without a data stream element in front, else the element
            int need = 0;
            if (len >= 2 && (bytes[a][0] >> 5) == 4) {
                const int n = bytes[a][1];
                need = n == 255 ? (len >= 3 ? 3 + 255 + bytes[a][2] : 0) : 2 + n;
                need = need > len ? 0 : need;                          // (malformed: the walk stops at the count)
            }
            const uint8_t *src = data + au_begin[a];
            for (int i = 3 + lane; i < need; i += 64) bytes[a][i] = src[i];
        }
        __syncthreads();
        if (lane == 0)
            for (int a = 0; a < n_aus; a++) pad::walk_au(st, c, bytes[a], au_len[a]);
    }
    __syncthreads();
    if (lane < STATE_WORDS) reinterpret_cast<uint4 *>(e.state_out)[lane] = reinterpret_cast<const uint4 *>(&st)[lane];
    if (lane < int(sizeof(pad::Label) / 4))
        reinterpret_cast<uint32_t *>(e.label)[lane] = reinterpret_cast<const uint32_t *>(&st.label)[lane];
    if (lane < int(sizeof(pad::Counters) / 4))
        reinterpret_cast<int32_t *>(e.result)[lane] = reinterpret_cast<const int32_t *>(&c)[lane];
}

}  // namespace

hipError_t launch_pad_labels(const PadEntry *entries, int n_entries, void *d_table, size_t table_bytes, hipStream_t stream) {
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || table_bytes < size_t(n_entries) * sizeof(PadEntry) || (reinterpret_cast<uintptr_t>(d_table) & 15))
        return hipErrorInvalidValue;
    for (int i = 0; i < n_entries; i++)
        if (entries[i].s < 1 || entries[i].s > 64 || entries[i].max_superframes < 0) return hipErrorInvalidValue;
    // (pageable memory: the copy has left `entries` when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, size_t(n_entries) * sizeof(PadEntry), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(pad_labels_kernel, dim3(unsigned(n_entries)), dim3(64), 0, stream, static_cast<const PadEntry *>(d_table));
    return hipGetLastError();
}

}  // namespace dabk
