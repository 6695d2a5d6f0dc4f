// mot_kernels.hip -- slideshow objects from the X-PAD of DAB+ access units (dabgpu_mot_slides_dev; contract: include/dabgpu.h,
// the control walk: include/dabgpu_mot_walk.h, shared with the host twin).
//
// One wave64 per followed sub-channel.  The fetch is pad_labels_kernel's: the status row a super-frame ahead, the three
// bytes in front of every access unit, then the PAD bytes of all of them into LDS.  Per access unit lane 0 runs the control
// walk over LDS (field walk, CRC, the data group's headers, the assembly's bookkeeping) and leaves copy orders in LDS; then
// all 64 lanes execute them one after the other: the reversed X-PAD bytes of a sub-field into the group buffer, a closed
// segment from the group buffer to its place, a completed object into its slot.  An order reads what the order before it
// wrote (through global memory, the same CU's L1), so a workgroup barrier with its fence stands between two orders.
#include <hip/hip_runtime.h>

#include "../../include/dabgpu_mot_walk.h"
#include "kernels.hpp"
#include "wave_copy.hpp"

namespace dabk {
namespace {

namespace pad = dabgpu_pad;
namespace mot = dabgpu_mot;

constexpr int MOT_MAX_AUS = 7;          // au_start[8] names at most seven
constexpr int MOT_AU_BYTES = 528;       // tag, count, escape count and at most 255 + 255 PAD bytes, rounded up to 16

static_assert(sizeof(mot::State) % 16 == 0 && sizeof(mot::Counters) % 4 == 0, "copied by words");
static_assert(sizeof(SuperframeStatus) == 64 && sizeof(FollowResult) == 32, "records of the follow call");

__global__ __launch_bounds__(64) void mot_slides_kernel(const MotEntry *table) {
    __shared__ mot::State st;
    __shared__ mot::Counters c;
    __shared__ mot::Orders ord;
    __shared__ int32_t row[16];
    __shared__ int32_t au_len[8], au_begin[8];
    __shared__ __attribute__((aligned(16))) uint8_t bytes[MOT_MAX_AUS][MOT_AU_BYTES];
    const MotEntry e = table[blockIdx.x];
    const int lane = threadIdx.x, s = e.s;
    constexpr int STATE_WORDS = int(sizeof(mot::State) / 16);
    if (lane < STATE_WORDS)
        reinterpret_cast<uint4 *>(&st)[lane] = e.state_in ? reinterpret_cast<const uint4 *>(e.state_in)[lane] : make_uint4(0u, 0u, 0u, 0u);
    int n_sf = reinterpret_cast<const FollowResult *>(e.follow)->n_superframes;
    n_sf = n_sf < 0 ? 0 : n_sf > e.max_superframes ? e.max_superframes : n_sf;
    if (lane < int(sizeof(mot::Counters) / 4)) reinterpret_cast<int32_t *>(&c)[lane] = 0;
    __syncthreads();
    if (lane == 0) mot::sanitize(st, e.body_capacity);
    uint8_t *arena = reinterpret_cast<uint8_t *>(e.arena), *slides = reinterpret_cast<uint8_t *>(e.slides);
    mot::Call call;
    call.body_capacity = e.body_capacity;
    call.max_slides = e.max_slides;
    call.slide_stride = e.slide_stride;
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
        call.superframe = k;
        for (int a = 0; a < n_aus; a++) {
            if (lane == 0) {
                call.au = a;
                mot::walk_au(st, c, ord, call, bytes[a], au_len[a]);
            }
            __syncthreads();
            const int n_orders = ord.n;
            for (int i = 0; i < n_orders; i++) {
                const mot::Order o = ord.o[i];
                if (o.kind == mot::ORDER_XPAD) {
                    for (int j = lane; j < o.len; j += 64) arena[o.dst + j] = bytes[a][o.src - j];
                } else if (o.kind == mot::ORDER_MOVE) {
                    wave_copy(arena + o.dst, arena + o.src, o.len, lane);
                } else if (o.kind == mot::ORDER_SLIDE) {
                    wave_copy(slides + o.dst, arena + o.src, o.len, lane);
                } else if (lane < mot::RECORD_BYTES / 4) {
                    reinterpret_cast<int32_t *>(slides + o.dst)[lane] = ord.record[o.src][lane];
                }
                __syncthreads();                                       // the next order, or the next walk, may read this one's bytes
            }
        }
    }
    __syncthreads();
    if (lane < STATE_WORDS) reinterpret_cast<uint4 *>(e.state_out)[lane] = reinterpret_cast<const uint4 *>(&st)[lane];
    if (lane < int(sizeof(mot::Counters) / 4))
        reinterpret_cast<int32_t *>(e.result)[lane] = reinterpret_cast<const int32_t *>(&c)[lane];
}

}  // namespace

hipError_t launch_mot_slides(const MotEntry *entries, int n_entries, void *d_table, size_t table_bytes, hipStream_t stream) {
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || table_bytes < size_t(n_entries) * sizeof(MotEntry) || (reinterpret_cast<uintptr_t>(d_table) & 15))
        return hipErrorInvalidValue;
    for (int i = 0; i < n_entries; i++) {
        const MotEntry &e = entries[i];
        if (e.s < 1 || e.s > 64 || e.max_superframes < 0 || e.max_slides < 0 || e.body_capacity < 0 ||
            e.body_capacity > mot::BODY_CAP_MAX || (e.max_slides > 0 && uint64_t(e.max_slides) * e.slide_stride >= (uint64_t(1) << 31)))
            return hipErrorInvalidValue;
    }
    // (pageable memory: the copy has left `entries` when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, size_t(n_entries) * sizeof(MotEntry), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(mot_slides_kernel, dim3(unsigned(n_entries)), dim3(64), 0, stream, static_cast<const MotEntry *>(d_table));
    return hipGetLastError();
}

}  // namespace dabk
