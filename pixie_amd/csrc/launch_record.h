// pixie_amd/csrc/launch_record.h -- the launch sites' side of launch_list.h: px_launch() launches a kernel as hipLaunchKernelGGL
// does or, while the calling thread has a recorder set (pixie_unet_forward_pair's plan walks), appends the launch to that list
// without touching the device; launch_rec() launches a record.  Group2<Args> is the parameter type of a grouped twin.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "launch_list.h"

namespace pixie {

// the calling thread's recorder, null = launch (defined in common.hip)
LaunchList*& launch_recorder();

// the one parameter of a grouped twin; argument set g of workgroup z is a[z / (gridDim.z / 2)] (wave-uniform: scalar loads)
template <class Args> struct Group2 { Args a[2]; };

template <class P> inline void launch_push_arg(LaunchRec& r, const P& v) {
    static_assert(std::is_trivially_copyable<P>::value, "kernel parameters are plain data");
    const size_t al = alignof(P);
    const size_t off = (r.args.size() + al - 1) / al * al;
    r.args.resize(off + sizeof(P), 0);
    std::memcpy(r.args.data() + off, &v, sizeof(P));
    r.offs.push_back((uint32_t)off);
}

template <class... P> constexpr size_t launch_args_stride() {   // sizeof of a struct whose members are P... in order
    size_t off = 0, ma = 1;
    ((off = (off + alignof(P) - 1) / alignof(P) * alignof(P) + sizeof(P), ma = alignof(P) > ma ? alignof(P) : ma), ...);
    return (off + ma - 1) / ma * ma;
}

template <class... P, class... A>
inline void px_launch_impl(void (*kern)(P...), const void* twin, dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... a) {
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    LaunchList* rec = launch_recorder();
    if (!rec) {
        hipLaunchKernelGGL(kern, grid, block, lds, st, std::forward<A>(a)...);
        return;
    }
    LaunchRec r;
    r.kernel = reinterpret_cast<const void*>(kern);
    r.twin = twin;
    r.grid[0] = grid.x; r.grid[1] = grid.y; r.grid[2] = grid.z;
    r.block[0] = block.x; r.block[1] = block.y; r.block[2] = block.z;
    r.lds = (uint32_t)lds;
    r.section = rec->section;
    (launch_push_arg<P>(r, static_cast<P>(a)), ...);
    r.arg_stride = (uint32_t)launch_args_stride<P...>();
    rec->recs.push_back(std::move(r));
}

// a kernel without a grouped twin
template <class... P, class... A>
inline void px_launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... a) {
    px_launch_impl(kern, nullptr, grid, block, lds, st, std::forward<A>(a)...);
}
// a kernel with one: Args is a struct of the kernel's parameters in order
template <class Args, class... P, class... A>
inline void px_launch_grouped(void (*kern)(P...), void (*twin)(Group2<Args>), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... a) {
    static_assert(sizeof(Args) == launch_args_stride<P...>(), "the twin's argument struct does not match the kernel's parameters");
    px_launch_impl(kern, reinterpret_cast<const void*>(twin), grid, block, lds, st, std::forward<A>(a)...);
}

inline hipError_t launch_rec(const LaunchRec& r, hipStream_t st) {
    void* argv[32];
    if (r.offs.size() > 32) return hipErrorInvalidValue;
    for (size_t i = 0; i < r.offs.size(); ++i) argv[i] = const_cast<unsigned char*>(r.args.data()) + r.offs[i];
    return hipLaunchKernel(r.kernel, dim3(r.grid[0], r.grid[1], r.grid[2]), dim3(r.block[0], r.block[1], r.block[2]), argv, r.lds, st);
}

}  // namespace pixie
