// pixie_amd/csrc/workspace_arena.h -- where the temporaries of one pass lie inside a caller-provided workspace: a head that one
// launch zeroes per pass (|x|max words, then the double targets of the statistics passes), and behind it a first-fit free list
// that places every activation, statistics buffer and split-K scratch.  The placement is a function of the sequence of requests
// only, which is what lets a dry run over fake addresses size the real pass.  Pure host code with no HIP in it:
// tests/test_unet_host.py compiles this header alone with g++ under ASan/UBSan and replays seeded request scripts against a model.
#pragma once
#include <cstdint>
#include <iterator>
#include <map>

namespace pixie::unet {

// First-fit free list over [0, capacity) in units of bytes; 256-byte granules.  `base == nullptr` = offsets only.
struct Arena {
    static constexpr int64_t kAlign = 256;
    char* base = nullptr;
    int64_t capacity = 0, peak = 0;
    std::map<int64_t, int64_t> free_;    // offset -> size, disjoint, coalesced
    std::map<int64_t, int64_t> used_;    // offset -> size

    void reset(char* b, int64_t cap) {
        base = b; capacity = cap; peak = 0;
        free_.clear(); used_.clear();
        free_[0] = cap;
    }
    int64_t alloc(int64_t bytes) {       // the lowest offset that fits, or -1 (and nothing changed) when no free range does
        bytes = (bytes + kAlign - 1) / kAlign * kAlign;
        if (bytes == 0) bytes = kAlign;
        for (auto it = free_.begin(); it != free_.end(); ++it) {
            if (it->second < bytes) continue;
            const int64_t off = it->first, rest = it->second - bytes;
            free_.erase(it);
            if (rest > 0) free_[off + bytes] = rest;
            used_[off] = bytes;
            if (off + bytes > peak) peak = off + bytes;
            return off;
        }
        return -1;
    }
    void release(int64_t off) {
        auto u = used_.find(off);
        if (u == used_.end()) return;
        int64_t size = u->second;
        used_.erase(u);
        auto next = free_.lower_bound(off);
        if (next != free_.end() && off + size == next->first) { size += next->second; next = free_.erase(next); }
        if (next != free_.begin()) {
            auto prev = std::prev(next);
            if (prev->first + prev->second == off) { prev->second += size; return; }
        }
        free_[off] = size;
    }
    template <class T> T* ptr(int64_t off) const { return reinterpret_cast<T*>(base + off); }   // dry run: small fake addresses, never dereferenced
};

struct Sized { int64_t bytes; int slots; int64_t zsum_doubles; };   // workspace bytes, |x|max words, pre-zeroed statistics doubles

// The head of the workspace: |x|max words at 0, the pre-zeroed doubles behind them, the arena behind both; each region a multiple
// of 256 bytes.  The sizing run adds arena_off to the arena's peak, the real pass clears [0, arena_off) and hands the rest to the arena.
struct HeadLayout {
    int64_t slots_off = 0, zsums_off, arena_off;
    static int64_t region(int64_t bytes) { return (bytes + 255) / 256 * 256; }
    explicit HeadLayout(const Sized& s) : zsums_off(region((int64_t)s.slots * 4)), arena_off(zsums_off + region(s.zsum_doubles * 8)) {}
};

}  // namespace pixie::unet
