// pixie_amd/csrc/scene_ingest.hip -- scene ingest: the body of a 3DGS checkpoint PLY, as it lies in the file, to the particles the
// solver loads and the static tail the rasteriser draws (PG/gs_simulation.py:403-438; per-Gaussian arithmetic: ingest_math.h).
//
// One pixie_scene_ingest call is the chain
//   [one small host-to-device copy: bounds initialised, rotation matrices, sim_area, column table]
//   ingest_classify_kernel   one lane per row: x, y, z, opacity through the column table -> class; writes the row's scan input
//                            (1 = selected, 1 << 32 = unselected, 0 = dropped) and folds the rotated positions of the selected rows
//                            into a bounding box: wave shuffles, LDS, then six order-preserving integer atomics per workgroup.
//                            min / max are exact, so the box does not depend on the order of arrival.
//   hipcub ExclusiveSum      over n + 1 packed counts (the last is 0): both destinations of every row, and the totals
//   ingest_finalise_kernel   one lane: the three counts, mean = (min + max) / 2, scale = 1 / max(max - min) in float32
//   [one stream synchronise: the host reads counts, scale, mean and refuses an empty or zero-extent selection]
//   ingest_emit_kernel<K>    one 256-thread workgroup per 64 rows.  The 64 rows are contiguous in the file body, so they come into
//                            LDS with 16-byte coalesced loads; wave 0 then does the geometry of one row per lane out of LDS, and all
//                            four waves copy the SH coefficients out of LDS transposed, (channel, coefficient) -> (coefficient,
//                            channel), consecutive lanes writing consecutive floats of the destination rows.  The compaction is
//                            stable: a row's destination is its scan value, selected rows at [0, n_sel), unselected after them.
// A row's class in the emit kernel is the difference of its two neighbouring scan values, i.e. exactly what the classify kernel
// decided; its rotated position comes from the same ingest_math.h function in both kernels, so the box and the mapped positions
// agree bit for bit (the selected positions span exactly [0.5, 1.5] on the longest axis before the z shift).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstdint>
#include <cstring>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "ingest_math.h"

using namespace pixie;
namespace im = pixie::ingest;

namespace {

constexpr int kBlock = 256;
constexpr int kTileRows = 64;             // rows per workgroup of the emit kernel: one wave does their geometry
constexpr int kGeoCols = 11;              // x y z opacity scale_0..2 rot_0..3
constexpr int kMaxCols = kGeoCols + 3 * 16;
constexpr int kMaxAttr = 254;             // 64 rows of n_attr floats + the tables fit the 64 KiB of LDS a launch gets by default
constexpr uint64_t kSelectedOne = 1ull, kUnselectedOne = 1ull << 32;

struct Result {
    int64_t counts[3];                    // selected, unselected, dropped
    float scale, mean[3], max_diff;
};

// start of the workspace: written by one host-to-device copy per call
struct Head {
    uint32_t lo[3], hi[3];                // bounding box of the selected rotated positions, order-preserving encoding
    uint32_t pad_[2];
    Result res;
    float rot[9 * im::kMaxRotations];
    float area[6];
    int32_t cols[kMaxCols + 5];
};
constexpr size_t kHeadBytes = 1024;
static_assert(sizeof(Head) <= kHeadBytes, "Head outgrew its slot");

struct Layout {
    size_t flags, offsets, scan_temp, scan_temp_bytes, total_bytes;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int make_layout(int64_t n, Layout& L) {
    L.flags = kHeadBytes;
    L.offsets = align256(L.flags + sizeof(uint64_t) * (size_t)(n + 1));
    L.scan_temp = align256(L.offsets + sizeof(uint64_t) * (size_t)(n + 1));
    L.scan_temp_bytes = 0;
    PX_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, L.scan_temp_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)(n + 1)));
    L.total_bytes = align256(L.scan_temp + L.scan_temp_bytes);
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

__global__ void __launch_bounds__(kBlock)
ingest_classify_kernel(int64_t n, int n_attr, const float* __restrict__ block, Head* __restrict__ head, int n_rot, int has_area,
                       float opacity_threshold, uint64_t* __restrict__ flags) {
    __shared__ float s_red[kBlock / 64][6];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
        const float* row = block + (size_t)i * n_attr;
        const float p[3] = {row[head->cols[0]], row[head->cols[1]], row[head->cols[2]]};
        const float opacity = im::activate_opacity(row[head->cols[3]]);
        float rp[3];
        im::rotate_position(p, head->rot, n_rot, rp);
        const int cls = im::classify(opacity, rp, opacity_threshold, has_area ? head->area : nullptr);
        flags[i] = cls == im::kSelected ? kSelectedOne : (cls == im::kUnselected ? kUnselectedOne : 0ull);
        if (cls == im::kSelected)
            for (int d = 0; d < 3; ++d) lo[d] = hi[d] = rp[d];
    } else if (i == n) {
        flags[n] = 0;                     // the scan runs over n + 1 counts
    }
    for (int d = 0; d < 3; ++d)
        for (int s = 32; s > 0; s >>= 1) {
            lo[d] = fminf(lo[d], __shfl_down(lo[d], s, 64));
            hi[d] = fmaxf(hi[d], __shfl_down(hi[d], s, 64));
        }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int d = 0; d < 3; ++d) { s_red[wave][d] = lo[d]; s_red[wave][3 + d] = hi[d]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int d = threadIdx.x;
        float v = s_red[0][d];
        for (int w = 1; w < kBlock / 64; ++w) v = d < 3 ? fminf(v, s_red[w][d]) : fmaxf(v, s_red[w][d]);
        if (d < 3) { if (v < INFINITY) atomicMin(&head->lo[d], ordered(v)); }
        else       { if (v > -INFINITY) atomicMax(&head->hi[d - 3], ordered(v)); }
    }
}

__global__ void ingest_finalise_kernel(int64_t n, const uint64_t* __restrict__ offsets, Head* __restrict__ head) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t total = offsets[n];
    const int64_t n_sel = (int64_t)(total & 0xffffffffull), n_unsel = (int64_t)(total >> 32);
    Result r;
    r.counts[0] = n_sel; r.counts[1] = n_unsel; r.counts[2] = n - n_sel - n_unsel;
    r.scale = 0.0f; r.mean[0] = r.mean[1] = r.mean[2] = 0.0f; r.max_diff = 0.0f;
    if (n_sel > 0) {
        float lo[3], hi[3];
        for (int d = 0; d < 3; ++d) { lo[d] = unordered(head->lo[d]); hi[d] = unordered(head->hi[d]); }
        r.max_diff = im::frame_of_bounds(lo, hi, r.mean, &r.scale);
    }
    head->res = r;
}

template <int K>
__global__ void __launch_bounds__(kBlock)
ingest_emit_kernel(int64_t n, int n_attr, const float* __restrict__ block, const Head* __restrict__ head,
                   const uint64_t* __restrict__ offsets, int n_rot, float z_shift, int64_t n_sel, float* __restrict__ out_pos,
                   float* __restrict__ out_cov, float* __restrict__ out_opacity, float* __restrict__ out_shs) {
    constexpr int kSh = 3 * K;            // floats of SH per row, in and out
    extern __shared__ float4 smem4[];     // [kTileRows * n_attr floats][kTileRows int32 destinations][kSh int32 source columns]
    float* tile = reinterpret_cast<float*>(smem4);
    int32_t* s_dst = reinterpret_cast<int32_t*>(tile + (size_t)kTileRows * n_attr);
    int32_t* s_shcol = s_dst + kTileRows;

    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
    const int rows = (int)(n - row0 < kTileRows ? n - row0 : kTileRows);

    int cls = im::kDropped;
    int32_t dst = -1;
    if (tid < rows) {
        const uint64_t o0 = offsets[row0 + tid], o1 = offsets[row0 + tid + 1];
        const uint64_t delta = o1 - o0;
        if (delta == kSelectedOne) { cls = im::kSelected; dst = (int32_t)(o0 & 0xffffffffull); }
        else if (delta == kUnselectedOne) { cls = im::kUnselected; dst = (int32_t)(n_sel + (int64_t)(o0 >> 32)); }
        s_dst[tid] = dst;
    }
    if (tid < kSh) {                      // output element (coefficient j, channel c) <- f_dc_c or f_rest_{c (K - 1) + j - 1}
        const int j = tid / 3, c = tid - 3 * j;
        s_shcol[tid] = head->cols[j == 0 ? kGeoCols + c : kGeoCols + 3 + c * (K - 1) + (j - 1)];
    }
    {   // the tile: rows * n_attr contiguous floats starting at a multiple of 256 bytes
        const float* src = block + (size_t)row0 * n_attr;
        const int cnt = rows * n_attr, n4 = cnt >> 2;
        const float4* src4 = reinterpret_cast<const float4*>(src);
        for (int j = tid; j < n4; j += kBlock) smem4[j] = src4[j];
        for (int j = 4 * n4 + tid; j < cnt; j += kBlock) tile[j] = src[j];
    }
    __syncthreads();

    if (cls != im::kDropped) {            // lanes of wave 0 only
        const float* row = tile + tid * n_attr;
        const int32_t* cols = head->cols;
        const float p[3] = {row[cols[0]], row[cols[1]], row[cols[2]]};
        const float ls[3] = {row[cols[4]], row[cols[5]], row[cols[6]]};
        const float q[4] = {row[cols[7]], row[cols[8]], row[cols[9]], row[cols[10]]};
        float c6[6], op[3], oc[6];
        im::covariance(ls, q, c6);
        if (cls == im::kSelected) {
            float rp[3], rc[6];
            im::rotate_position(p, head->rot, n_rot, rp);
            im::map_position(rp, head->res.mean, head->res.scale, z_shift, op);
            im::rotate_covariance(c6, head->rot, n_rot, rc);
            im::map_covariance(rc, head->res.scale, oc);
        } else {
            for (int d = 0; d < 3; ++d) op[d] = p[d];
            for (int d = 0; d < 6; ++d) oc[d] = c6[d];
        }
        for (int d = 0; d < 3; ++d) out_pos[(size_t)dst * 3 + d] = op[d];
        for (int d = 0; d < 6; ++d) out_cov[(size_t)dst * 6 + d] = oc[d];
        out_opacity[dst] = im::activate_opacity(row[cols[3]]);
    }

    for (int idx = tid; idx < rows * kSh; idx += kBlock) {
        const int r = idx / kSh, e = idx - r * kSh;
        const int32_t d = s_dst[r];
        if (d >= 0) out_shs[(size_t)d * kSh + e] = tile[r * n_attr + s_shcol[e]];
    }
}

template <int K>
hipError_t launch_emit(const pixie_ingest_desc* d, const Head* head, const uint64_t* offsets, int64_t n_sel, hipStream_t st) {
    const size_t lds = sizeof(float) * (size_t)kTileRows * d->n_attr + sizeof(int32_t) * (kTileRows + 3 * K);
    hipLaunchKernelGGL(ingest_emit_kernel<K>, dim3((unsigned)cdiv(d->n, kTileRows)), dim3(kBlock), lds, st, d->n, d->n_attr, d->d_block, head,
                       offsets, d->n_rotations, d->z_shift, n_sel, d->d_pos, d->d_cov, d->d_opacity, d->d_shs);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int64_t pixie_scene_ingest_workspace_bytes(int64_t n) {
    if (n < 0 || n > (int64_t)INT_MAX - 1) {
        set_error("pixie_scene_ingest_workspace_bytes: n %lld outside [0, 2^31 - 2]", (long long)n);
        return -1;
    }
    Layout L;
    if (make_layout(n, L)) return -1;
    return (int64_t)L.total_bytes;
}

int pixie_scene_ingest(const pixie_ingest_desc* d, int64_t counts_out[3], float scale_out[1], float mean_out[3], void* stream) {
    PX_REQUIRE(d, "pixie_scene_ingest: null descriptor");
    if (counts_out) counts_out[0] = counts_out[1] = counts_out[2] = 0;
    PX_REQUIRE(d->n >= 0, "pixie_scene_ingest: n %lld < 0", (long long)d->n);
    if (d->n > (int64_t)INT_MAX - 1) {
        set_error("pixie_scene_ingest: %lld Gaussians exceed the 2^31 - 2 one call takes", (long long)d->n);
        return PIXIE_INGEST_TOO_MANY_ROWS;
    }
    if (d->n_rotations > im::kMaxRotations) {
        set_error("pixie_scene_ingest: %d rotations exceed the %d one call takes", d->n_rotations, im::kMaxRotations);
        return PIXIE_INGEST_TOO_MANY_ROTATIONS;
    }
    PX_REQUIRE(d->n_rotations >= 0, "pixie_scene_ingest: n_rotations %d < 0", d->n_rotations);
    PX_REQUIRE(d->sh_degree >= 0 && d->sh_degree <= 3, "pixie_scene_ingest: sh_degree %d outside 0..3", d->sh_degree);
    PX_REQUIRE(d->n_attr >= 1 && d->n_attr <= kMaxAttr, "pixie_scene_ingest: n_attr %d outside 1..%d", d->n_attr, kMaxAttr);
    PX_REQUIRE(d->columns, "pixie_scene_ingest: null column table");
    const int K = (d->sh_degree + 1) * (d->sh_degree + 1);
    const int n_cols = kGeoCols + 3 * K;

    Head host;
    memset(&host, 0, sizeof host);
    for (int k = 0; k < 3; ++k) { host.lo[k] = 0xffffffffu; host.hi[k] = 0u; }
    for (int k = 0; k < n_cols; ++k) {
        PX_REQUIRE(d->columns[k] >= 0 && d->columns[k] < d->n_attr, "pixie_scene_ingest: column table entry %d is %d, outside [0, %d)", k,
                   d->columns[k], d->n_attr);
        host.cols[k] = d->columns[k];
    }
    memcpy(host.rot, d->rotations, sizeof(float) * 9 * (size_t)d->n_rotations);
    memcpy(host.area, d->sim_area, sizeof host.area);
    if (d->n == 0) {
        set_error("pixie_scene_ingest: no Gaussian is selected (the file has none)");
        return PIXIE_INGEST_NO_SELECTION;
    }
    PX_REQUIRE(d->d_block && d->d_pos && d->d_cov && d->d_opacity && d->d_shs,
               "pixie_scene_ingest: null pointer (d_block, d_pos, d_cov, d_opacity and d_shs are required)");
    PX_REQUIRE(((uintptr_t)d->d_block & 15) == 0, "pixie_scene_ingest: d_block must be 16-byte aligned");
    Layout L;
    if (make_layout(d->n, L)) return 1;
    PX_REQUIRE(d->d_workspace && d->workspace_bytes >= (int64_t)L.total_bytes,
               "pixie_scene_ingest: workspace of %lld bytes is smaller than the %lld bytes that %lld Gaussians need",
               (long long)d->workspace_bytes, (long long)L.total_bytes, (long long)d->n);
    PX_REQUIRE(((uintptr_t)d->d_workspace & 15) == 0, "pixie_scene_ingest: d_workspace must be 16-byte aligned");

    hipStream_t st = as_stream(stream);
    char* ws = (char*)d->d_workspace;
    Head* head = (Head*)ws;
    uint64_t* flags = (uint64_t*)(ws + L.flags);
    uint64_t* offsets = (uint64_t*)(ws + L.offsets);
    const int64_t n = d->n;

    PX_CHECK_HIP(hipMemcpyAsync(head, &host, sizeof host, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ingest_classify_kernel, dim3((unsigned)cdiv(n + 1, kBlock)), dim3(kBlock), 0, st, n, d->n_attr, d->d_block, head,
                       d->n_rotations, d->has_sim_area, d->opacity_threshold, flags);
    PX_CHECK_HIP(hipGetLastError());
    size_t tb = L.scan_temp_bytes;
    PX_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(ws + L.scan_temp, tb, (const uint64_t*)flags, offsets, (int)(n + 1), st));
    hipLaunchKernelGGL(ingest_finalise_kernel, dim3(1), dim3(64), 0, st, n, offsets, head);
    PX_CHECK_HIP(hipGetLastError());
    Result res;
    PX_CHECK_HIP(hipMemcpyAsync(&res, &head->res, sizeof res, hipMemcpyDeviceToHost, st));
    PX_CHECK_HIP(hipStreamSynchronize(st));          // the only one of the call
    if (counts_out) for (int k = 0; k < 3; ++k) counts_out[k] = res.counts[k];
    if (scale_out) scale_out[0] = res.scale;
    if (mean_out) for (int k = 0; k < 3; ++k) mean_out[k] = res.mean[k];
    if (res.counts[0] == 0) {
        set_error("pixie_scene_ingest: no Gaussian is selected (%lld unselected, %lld dropped)", (long long)res.counts[1], (long long)res.counts[2]);
        return PIXIE_INGEST_NO_SELECTION;
    }
    if (!(res.max_diff > 0.0f)) {
        set_error("pixie_scene_ingest: the %lld selected Gaussians have zero extent, so the solver frame's scale 1 / max(max - min) is not finite",
                  (long long)res.counts[0]);
        return PIXIE_INGEST_ZERO_EXTENT;
    }
    hipError_t e = hipSuccess;
    switch (K) {
        case 1: e = launch_emit<1>(d, head, offsets, res.counts[0], st); break;
        case 4: e = launch_emit<4>(d, head, offsets, res.counts[0], st); break;
        case 9: e = launch_emit<9>(d, head, offsets, res.counts[0], st); break;
        default: e = launch_emit<16>(d, head, offsets, res.counts[0], st); break;
    }
    PX_CHECK_HIP(e);
    return 0;
}

}  // extern "C"
