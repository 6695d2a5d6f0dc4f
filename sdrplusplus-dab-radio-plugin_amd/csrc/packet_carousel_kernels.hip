// packet_carousel_kernels.hip -- packet-mode MOT directory carousels to objects (dabgpu_packet_carousel_dev; contract and
// code: include/dabgpu_mot_carousel.h, shared with the host twin).  The scan launch is packet_kernels.hip's, unchanged; the
// walk is packet_walk_body.hpp's kernel with the sink below: behind the orders of a followed packet come the directory check,
// when that packet completed the directory, and one emission attempt, each control in lane 0 and its orders by the whole wave.
#include "packet_walk_body.hpp"

namespace dabk {
namespace {

static_assert(sizeof(car::State) % 16 == 0 && sizeof(car::Counters) % 4 == 0, "copied by words");

// directory mode.  The LDS record of this instantiation: the state 6448 bytes (packet state 176, directory part, 32 body
// parts of 64, the index of 256 entries of 16, the delivered bits), counters 256, orders 464, packet 96: 7.1 KiB per
// workgroup of one wave, 22 workgroups a CU by LDS; the launch has one workgroup per entry, so LDS does not bound occupancy
// before the entry count does.  Control is lane 0 over LDS; the directory check reads the directory's bytes in the arena
// (global memory) serially: N <= 256 dependent steps, once per directory that completes.  Behind it the stale assemblies are
// found and emptied by a lane each.  The searches of the index and of the assemblies for a segment's id stay in lane 0.
struct CarouselWalk {
    using State = car::State;
    using Counters = car::Counters;
    car::Call call;
    __device__ __forceinline__ CarouselWalk(const PacketEntry &e, const CarouselExtra *x) {
        call.directory_capacity = x->directory_capacity;
        call.assemblies = x->assemblies;
        call.object_capacity = e.body_capacity;
        call.max_objects = e.max_slides;
        call.object_stride = e.slide_stride;
        call.frame = call.slot = 0;
        call.deferred = 0;
    }
    __device__ __forceinline__ static uint8_t *directory(const CarouselExtra *x) { return reinterpret_cast<uint8_t *>(x->directory); }
    __device__ __forceinline__ static pkt::Counters &head(Counters &c) { return c.head; }
    __device__ __forceinline__ void sanitize(State &st) const { car::sanitize(st, call.directory_capacity, call.assemblies, call.object_capacity); }
    __device__ __forceinline__ void follow(State &st, Counters &c, mot::Orders &ord, const uint8_t *bytes, int L, int k, int pos) {
        call.frame = k;
        call.slot = pos;
        car::follow_packet(st, c, ord, call, bytes, L);
    }
    // (entered by the whole wave behind a barrier: st and ord are LDS, every lane sees the same)
    __device__ __forceinline__ void behind(State &st, Counters &c, mot::Orders &ord, const uint8_t *bytes, uint8_t *arena, uint8_t *out, uint8_t *dir,
                           int lane) {
        if (st.check_pending) {
            __syncthreads();                                           // (every lane has read check_pending)
            if (lane == 0) car::check_directory_phase(st, c, ord, arena + car::DIRECTORY_OFF);
            __syncthreads();
            // it has become current exactly when the check left the order that copies it out; then a lane per assembly
            // searches the index for its id, and those that are not listed are emptied, each by its own lane
            if (ord.n > 0) {
                const bool stale = lane < call.assemblies && car::body_is_stale(st, lane);
                const uint64_t all = __ballot(stale);
                if (stale) car::empty_body(st.body[lane]);
                if (lane == 0) c.objects_stale += __popcll(static_cast<unsigned long long>(all));
                __syncthreads();
            }
            execute_orders(ord, bytes, arena, out, dir, lane);
        }
        if (lane == 0) car::emit_attempt(st, c, ord, call);
        __syncthreads();
        execute_orders(ord, bytes, arena, out, dir, lane);
    }
    __device__ __forceinline__ static void finish(const State &st, Counters &c) { car::finish(st, c); }
};

}  // namespace

hipError_t launch_carousel_walk(const PacketEntry *d_table, const CarouselExtra *d_extras, int n_entries, int n_cifs, hipStream_t stream) {
    hipLaunchKernelGGL(packet_walk_kernel<CarouselWalk>, dim3(unsigned(n_entries)), dim3(64), 0, stream, d_table, d_extras, n_cifs);
    return hipGetLastError();
}

}  // namespace dabk
