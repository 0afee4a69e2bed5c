// pixie_amd/csrc/launch_list.h -- a forward pass as data: the record of one kernel launch, the list a plan walk appends to
// instead of launching (launch_record.h), and merge_pair(), which interleaves the lists of two networks that run on one stream.
// Pure host code with no HIP in it: g++ compiles it alone for tests/test_launch_list_host.py.
//
// Why: below full resolution a U-Net pass is a long dependent chain of short launches (conv -> split-K reduce -> finalise), and the
// two networks of a scene walk the same chain one after the other.  Two launches at the same position of the two chains that run the
// same kernel instantiation on the same grid can go out as ONE launch of that kernel's grouped twin: the same code behind one more
// grid dimension that selects the argument set.  Every workgroup computes what it computed before; only the launch that carries it
// changes, so the results are the two single launches' bit for bit.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pixie {

enum LaunchSection : int { SEC_FULLRES = 0, SEC_INNER = 1 };   // inner: the output grid is below the network's input resolution

struct LaunchRec {
    const void* kernel = nullptr;     // host-side identity of the __global__ function
    // The grouped twin, or null: a kernel with ONE parameter, struct { Args a[2]; }, where Args holds this kernel's parameters in
    // order (so sizeof(Args) == arg_stride), launched with grid z doubled; workgroup z runs argument set z / (gridDim.z / 2) as
    // workgroup z % (gridDim.z / 2) of the single form.
    const void* twin = nullptr;
    uint32_t grid[3] = {1, 1, 1}, block[3] = {1, 1, 1};
    uint32_t lds = 0;                 // dynamic LDS bytes
    int section = SEC_FULLRES;
    int net = 0;                      // which list the launch came from; -1 for a grouped launch
    std::vector<unsigned char> args;  // the parameters, laid out as a C struct of them
    std::vector<uint32_t> offs;       // offset of each parameter in args
    uint32_t arg_stride = 0;          // args.size() rounded up to the widest parameter's alignment
};

struct LaunchList {
    std::vector<LaunchRec> recs;
    int section = SEC_FULLRES;        // the mark the next appended record gets
};

inline bool launch_groupable(const LaunchRec& a, const LaunchRec& b) {
    return a.kernel == b.kernel && a.twin != nullptr && a.twin == b.twin && a.lds == b.lds && a.arg_stride == b.arg_stride &&
           a.args.size() == b.args.size() && std::memcmp(a.grid, b.grid, sizeof a.grid) == 0 && std::memcmp(a.block, b.block, sizeof a.block) == 0;
}

// one launch of a.twin that does the work of a, then b
inline LaunchRec launch_group(const LaunchRec& a, const LaunchRec& b) {
    LaunchRec g;
    g.kernel = a.twin;
    std::memcpy(g.grid, a.grid, sizeof g.grid);
    std::memcpy(g.block, a.block, sizeof g.block);
    g.grid[2] *= 2;
    g.lds = a.lds;
    g.section = a.section;
    g.net = -1;
    g.args.assign((size_t)2 * a.arg_stride, 0);
    std::memcpy(g.args.data(), a.args.data(), a.args.size());
    std::memcpy(g.args.data() + a.arg_stride, b.args.data(), b.args.size());
    g.offs.assign(1, 0u);
    g.arg_stride = 2 * a.arg_stride;
    return g;
}

// The launches of two passes on one stream: list 0's full-resolution encoder section, list 1's, the two inner sections zipped
// (position by position; a pair that launch_groupable() accepts becomes one grouped launch, any other goes out as its two launches,
// list 0's first; what the longer section has beyond the shorter follows), list 0's decoder section, list 1's.  A list's inner
// section is the run from its first SEC_INNER record to its last.  Each list's launches keep their own order and appear exactly
// once; lists that differ in length or shape only group less.  *n_grouped: the number of grouped launches; group = false: none.
inline std::vector<LaunchRec> merge_pair(const LaunchList& l0, const LaunchList& l1, int* n_grouped = nullptr, bool group = true) {
    const LaunchList* ls[2] = {&l0, &l1};
    size_t lo[2], hi[2];              // the inner section is [lo, hi)
    for (int k = 0; k < 2; ++k) {
        const std::vector<LaunchRec>& r = ls[k]->recs;
        lo[k] = hi[k] = r.size();
        for (size_t i = 0; i < r.size(); ++i)
            if (r[i].section == SEC_INNER) { if (lo[k] == r.size()) lo[k] = i; hi[k] = i + 1; }
        if (lo[k] == r.size()) lo[k] = hi[k] = r.size();   // no inner section: everything is the encoder section
    }
    std::vector<LaunchRec> out;
    out.reserve(l0.recs.size() + l1.recs.size());
    auto put = [&](int k, size_t i) { out.push_back(ls[k]->recs[i]); out.back().net = k; };
    int grouped = 0;
    for (int k = 0; k < 2; ++k)
        for (size_t i = 0; i < lo[k]; ++i) put(k, i);
    const size_t n0 = hi[0] - lo[0], n1 = hi[1] - lo[1];
    for (size_t i = 0; i < (n0 > n1 ? n0 : n1); ++i) {
        if (group && i < n0 && i < n1 && launch_groupable(l0.recs[lo[0] + i], l1.recs[lo[1] + i])) {
            out.push_back(launch_group(l0.recs[lo[0] + i], l1.recs[lo[1] + i]));
            ++grouped;
            continue;
        }
        if (i < n0) put(0, lo[0] + i);
        if (i < n1) put(1, lo[1] + i);
    }
    for (int k = 0; k < 2; ++k)
        for (size_t i = hi[k]; i < ls[k]->recs.size(); ++i) put(k, i);
    if (n_grouped) *n_grouped = grouped;
    return out;
}

}  // namespace pixie
