// pixie_amd/csrc/knn.hip -- distCUDA2 of simple-knn: for every point of a cloud, the mean squared distance to its three nearest
// other points (gaussian-splatting/scene/gaussian_model.py:create_from_pcd initialises the Gaussians' scales from it).  The
// arithmetic is knn_math.h; this file is built with -ffp-contract=off, so the result is bit-equal to a float32 brute force with the
// same expression order, whatever the order of the input rows.
//
// One pixie_knn_mean_dist2 call is the chain
//   [two memsets: the bounding box's order-preserving integer encoding]
//   knn_bounds_kernel    one lane per point: wave shuffles, LDS, then six integer atomicMin / atomicMax per workgroup.  min and
//                        max are exact, so the box does not depend on the order of arrival; no host round trip.
//   knn_morton_kernel    one lane per point: 30-bit Morton code inside that box, and the identity permutation
//   hipcub SortPairs     30 bits, stable
//   knn_gather_kernel    one wave per group of 64 consecutive sorted points: (x, y, z, original index) in sorted order, 16 bytes a
//                        point, and the group's bounding box (wave shuffles)
//   knn_search_kernel    one wave per group, one point per lane, three best distances in registers.  The wave first takes its own
//                        64 points, then walks ALL groups 64 at a time: lane l bounds group c + l against the wave's own box
//                        (box_box_dist2) and a ballot leaves the groups that can still hold a closer point for some lane, i.e.
//                        those whose bound does not exceed the largest third-best distance in the wave.  That maximum only
//                        shrinks, so it is taken again before each surviving group is read.  A surviving group's points come
//                        in with one coalesced 1 KiB load, a point per lane, and reach every lane as wave-uniform operands
//                        (v_readlane with a constant lane: no LDS, no barrier); every lane updates its own three registers.
//                        Control flow is wave-uniform throughout and every loop is counted, so no input can make it spin.
// There are no floating-point atomics and no order-dependent sums: the output is bit-identical from run to run.
// Groups of 64 (rather than simple-knn's boxes of 1024 scanned by divergent lanes) keep the boxes tight -- fewer distances per
// point -- and make the wave the unit of both pruning and staging.  Cost of the walk: ceil(groups / 64) ballots per wave.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cfloat>
#include <cstdint>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "knn_math.h"

using namespace pixie;
namespace km = pixie::knn;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSortBits = 30;
constexpr size_t kHeadBytes = 256;

struct Head {
    uint32_t lo[3], hi[3];                // bounding box of the cloud, order-preserving encoding
};

struct Layout {
    size_t codes, codes_sorted, idx, idx_sorted, sorted, boxes, sort_temp, sort_temp_bytes, total_bytes;
    int groups;
};

size_t take(size_t& cursor, size_t bytes) {
    const size_t at = cursor;
    cursor = (cursor + bytes + 255) & ~(size_t)255;
    return at;
}

int make_layout(int64_t n, Layout& L) {
    L.groups = (int)((n + km::kGroup - 1) / km::kGroup);
    size_t cur = kHeadBytes;
    L.codes = take(cur, sizeof(uint32_t) * (size_t)n);
    L.codes_sorted = take(cur, sizeof(uint32_t) * (size_t)n);
    L.idx = take(cur, sizeof(uint32_t) * (size_t)n);
    L.idx_sorted = take(cur, sizeof(uint32_t) * (size_t)n);
    L.sorted = take(cur, sizeof(uint4) * (size_t)L.groups * km::kGroup);
    L.boxes = take(cur, sizeof(float) * 6 * (size_t)L.groups);
    // The sort's temporary storage is reserved by a bound, not asked of hipcub: the size query of the library needs a device for
    // all but small inputs, and a scratch size should be a pure function of n.  rocPRIM's onesweep takes a second copy of keys and
    // values (8 n bytes), 256 lookback words per block of at least 1024 items (<= n bytes) and a few KiB of digit counters.  The
    // call asks hipcub for the actual need and refuses if it ever exceeds this reservation.
    L.sort_temp_bytes = 12 * (size_t)n + (64u << 10);
    L.sort_temp = take(cur, L.sort_temp_bytes);
    L.total_bytes = cur;
    return 0;
}

// float <-> unsigned with the same order (for atomicMin / atomicMax on floats of either sign)
__device__ __forceinline__ uint32_t ordered(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__device__ __forceinline__ float wave_min(float v) {
    for (int s = 32; s > 0; s >>= 1) v = fminf(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
    return v;
}
// lane `j` of v for every lane; j is wave-uniform
__device__ __forceinline__ float lane_value(float v, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

__global__ void __launch_bounds__(kBlock)
knn_bounds_kernel(int n, const float* __restrict__ points, Head* __restrict__ head) {
    __shared__ float s_red[kWaves][6];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n)
        for (int d = 0; d < 3; ++d) lo[d] = hi[d] = points[(size_t)i * 3 + d];
    for (int d = 0; d < 3; ++d) { lo[d] = wave_min(lo[d]); hi[d] = wave_max(hi[d]); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int d = 0; d < 3; ++d) { s_red[wave][d] = lo[d]; s_red[wave][3 + d] = hi[d]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int d = threadIdx.x;
        float v = s_red[0][d];
        for (int w = 1; w < kWaves; ++w) v = d < 3 ? fminf(v, s_red[w][d]) : fmaxf(v, s_red[w][d]);
        if (d < 3) { if (v < INFINITY) atomicMin(&head->lo[d], ordered(v)); }
        else       { if (v > -INFINITY) atomicMax(&head->hi[d - 3], ordered(v)); }
    }
}

__global__ void __launch_bounds__(kBlock)
knn_morton_kernel(int n, const float* __restrict__ points, const Head* __restrict__ head, uint32_t* __restrict__ codes,
                  uint32_t* __restrict__ idx) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float lo[3], hi[3], p[3];
    for (int d = 0; d < 3; ++d) { lo[d] = unordered(head->lo[d]); hi[d] = unordered(head->hi[d]); p[d] = points[(size_t)i * 3 + d]; }
    codes[i] = km::morton3(p, lo, hi);
    idx[i] = (uint32_t)i;
}

// sorted: groups * 64 records (the tail of the last group is never read); boxes: [6][groups] = lo x y z, hi x y z
__global__ void __launch_bounds__(kBlock)
knn_gather_kernel(int n, int groups, const float* __restrict__ points, const uint32_t* __restrict__ idx_sorted,
                  uint4* __restrict__ sorted, float* __restrict__ boxes) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (g >= groups) return;                                  // the whole wave
    const int i = g * km::kGroup + lane;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
        const uint32_t src = idx_sorted[i];
        float p[3];
        for (int d = 0; d < 3; ++d) lo[d] = hi[d] = p[d] = points[(size_t)src * 3 + d];
        sorted[i] = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]), src);
    }
    for (int d = 0; d < 3; ++d) { lo[d] = wave_min(lo[d]); hi[d] = wave_max(hi[d]); }
    if (lane == 0)
        for (int d = 0; d < 3; ++d) { boxes[(size_t)d * groups + g] = lo[d]; boxes[(size_t)(3 + d) * groups + g] = hi[d]; }
}

// Every lane takes the `cnt` points that lanes 0 .. cnt - 1 hold in (sx, sy, sz) into its three best.  kSelf: the points are the
// wave's own, and a lane skips itself (by index: a coincident other point still counts, at distance 0).
template <bool kSelf>
__device__ __forceinline__ void take_group(float sx, float sy, float sz, int cnt, int lane, float px, float py, float pz, float& b0,
                                           float& b1, float& b2) {
    if (cnt == km::kGroup) {
#pragma unroll
        for (int j = 0; j < km::kGroup; ++j) {
            float d = km::dist2(px, py, pz, lane_value(sx, j), lane_value(sy, j), lane_value(sz, j));
            if (kSelf && j == lane) d = FLT_MAX;              // leaves the three best as they are
            km::insert3(d, b0, b1, b2);
        }
    } else {                                                  // the cloud's last group
        for (int j = 0; j < cnt; ++j) {
            float d = km::dist2(px, py, pz, lane_value(sx, j), lane_value(sy, j), lane_value(sz, j));
            if (kSelf && j == lane) d = FLT_MAX;
            km::insert3(d, b0, b1, b2);
        }
    }
}

__global__ void __launch_bounds__(kBlock)
knn_search_kernel(int n, int groups, const uint4* __restrict__ sorted, const float* __restrict__ boxes, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (g >= groups) return;                                  // the whole wave
    const int i = g * km::kGroup + lane;
    const bool valid = i < n;
    uint4 me = make_uint4(0u, 0u, 0u, 0u);
    if (valid) me = sorted[i];
    const float px = __uint_as_float(me.x), py = __uint_as_float(me.y), pz = __uint_as_float(me.z);
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;
    const int own = n - g * km::kGroup < km::kGroup ? n - g * km::kGroup : km::kGroup;
    take_group<true>(px, py, pz, own, lane, px, py, pz, b0, b1, b2);

    float glo[3], ghi[3];
    for (int d = 0; d < 3; ++d) { glo[d] = boxes[(size_t)d * groups + g]; ghi[d] = boxes[(size_t)(3 + d) * groups + g]; }

    for (int c = 0; c < groups; c += 64) {                    // counted: ceil(groups / 64) rounds
        const int b = c + lane;
        float bound = INFINITY;
        if (b < groups && b != g) {
            float blo[3], bhi[3];
            for (int d = 0; d < 3; ++d) { blo[d] = boxes[(size_t)d * groups + b]; bhi[d] = boxes[(size_t)(3 + d) * groups + b]; }
            bound = km::box_box_dist2(glo, ghi, blo, bhi);
        }
        float reach = wave_max(valid ? b2 : 0.0f);            // no lane of this wave can use a point further away than this
        unsigned long long live = __ballot(bound <= reach);
        while (live) {                                        // at most 64 rounds: one bit is cleared in each
            const int j = __ffsll((long long)live) - 1;
            live &= live - 1;
            reach = wave_max(valid ? b2 : 0.0f);
            if (!(lane_value(bound, j) <= reach)) continue;
            const int src = c + j;
            const int cnt = n - src * km::kGroup < km::kGroup ? n - src * km::kGroup : km::kGroup;
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            if (lane < cnt) q = sorted[(size_t)src * km::kGroup + lane];
            take_group<false>(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), cnt, lane, px, py, pz, b0, b1, b2);
        }
    }
    if (valid) out[me.w] = km::mean3(b0, b1, b2);
}

}  // namespace

extern "C" {

int64_t pixie_knn_mean_dist2_scratch_bytes(int64_t n) {
    if (n < 0 || n > km::kMaxPoints) {
        set_error("pixie_knn_mean_dist2_scratch_bytes: n %lld outside [0, 2^24]", (long long)n);
        return -1;
    }
    Layout L;
    if (make_layout(n, L)) return -1;
    return (int64_t)L.total_bytes;
}

int pixie_knn_mean_dist2(const float* d_points, int64_t n, void* d_scratch, int64_t scratch_bytes, float* d_out, void* stream) {
    PX_REQUIRE(n >= 0, "pixie_knn_mean_dist2: n %lld < 0", (long long)n);
    PX_REQUIRE(n <= km::kMaxPoints, "pixie_knn_mean_dist2: %lld points exceed the 2^24 one call takes", (long long)n);
    if (n == 0) return 0;
    PX_REQUIRE(d_points && d_out, "pixie_knn_mean_dist2: null pointer (d_points and d_out are required)");
    Layout L;
    if (make_layout(n, L)) return 1;
    PX_REQUIRE(d_scratch && scratch_bytes >= (int64_t)L.total_bytes,
               "pixie_knn_mean_dist2: scratch of %lld bytes is smaller than the %lld bytes that %lld points need",
               (long long)scratch_bytes, (long long)L.total_bytes, (long long)n);
    PX_REQUIRE(((uintptr_t)d_scratch & 15) == 0, "pixie_knn_mean_dist2: d_scratch must be 16-byte aligned");

    hipStream_t st = as_stream(stream);
    char* ws = (char*)d_scratch;
    Head* head = (Head*)ws;
    uint32_t* codes = (uint32_t*)(ws + L.codes);
    uint32_t* codes_sorted = (uint32_t*)(ws + L.codes_sorted);
    uint32_t* idx = (uint32_t*)(ws + L.idx);
    uint32_t* idx_sorted = (uint32_t*)(ws + L.idx_sorted);
    uint4* sorted = (uint4*)(ws + L.sorted);
    float* boxes = (float*)(ws + L.boxes);
    const int ni = (int)n;

    PX_CHECK_HIP(hipMemsetAsync(head->lo, 0xff, sizeof head->lo, st));
    PX_CHECK_HIP(hipMemsetAsync(head->hi, 0x00, sizeof head->hi, st));
    hipLaunchKernelGGL(knn_bounds_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, ni, d_points, head);
    PX_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(knn_morton_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, ni, d_points, head, codes, idx);
    PX_CHECK_HIP(hipGetLastError());
    size_t tb = 0;
    PX_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint32_t*)codes, codes_sorted, (const uint32_t*)idx, idx_sorted, ni, 0,
                                                    kSortBits, st));
    PX_REQUIRE(tb <= L.sort_temp_bytes, "pixie_knn_mean_dist2: the sort needs %zu bytes of temporary storage for %d points, more than the %zu reserved",
               tb, ni, L.sort_temp_bytes);
    PX_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws + L.sort_temp, tb, (const uint32_t*)codes, codes_sorted, (const uint32_t*)idx, idx_sorted,
                                                    ni, 0, kSortBits, st));
    hipLaunchKernelGGL(knn_gather_kernel, dim3((unsigned)cdiv(L.groups, kWaves)), dim3(kBlock), 0, st, ni, L.groups, d_points, idx_sorted,
                       sorted, boxes);
    PX_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(knn_search_kernel, dim3((unsigned)cdiv(L.groups, kWaves)), dim3(kBlock), 0, st, ni, L.groups, sorted, boxes, d_out);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
