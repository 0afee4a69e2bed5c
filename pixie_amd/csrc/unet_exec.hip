// pixie_amd/csrc/unet_exec.hip -- one U-Net as a C-ABI handle: pixie_unet_{create,set_param,workspace_bytes,forward,destroy}.
//
// Replaces, for one network, what the reference does with an nn.Module: construction (MyUNetModel.__init__,
// WG/models/module/diffusion_network.py:712-873; FeatureProjector :534-589; the wrappers trainer/training_discrete.py:50-88,
// trainer/training_continuous_mse.py:48-89), load_state_dict (keys in registration order) and forward (:875-935).  A
// forward pass is a fixed sequence of ~400 launches of the operators of section (A); this file owns that sequence, so a
// caller in any language pays ONE foreign call per scene instead of ~400 plus ~600 temporary allocations, and the sequence
// is capturable into a HIP graph (it allocates nothing and never synchronises after the first call).
//
// Memory: every temporary of a pass -- activations, statistics, split-K scratch -- lives in ONE caller-provided workspace
// (pixie_unet_workspace_bytes); a first-fit free list places them, tensors return their range when the last consumer has
// been launched (everything is ordered on one stream, so reuse is safe).  The placement is a function of the shapes only:
// the dry run that sizes the workspace and the real pass take the same decisions.  The handle owns only the re-packed
// weights.  The operators are called through the same extern "C" entry points a foreign caller would use; the launch order
// equals pixie_amd/unet.py: UNetRunner.forward, so both executors produce bit-identical tensors (tests/test_unet_hip.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "conv_launch.h"
#include "conv_plan.h"
#include "launch_record.h"

namespace pixie {
// internal entry points of unet_ops.hip (the launches of pixie_channel_stats / pixie_norm_finalize without their set-up work)
int channel_stats_prezeroed(const float* d_x, int channels, int64_t spatial, double* d_sums, uint32_t* d_amax, hipStream_t st);
int norm_finalize_cat(const double* d_sums0, int c0, const double* d_sums1, int c1, int64_t spatial, int mode, int groups, double eps,
                      const float* d_weight, const float* d_bias, float* d_a, float* d_b, hipStream_t st);
namespace {

enum { ACT_NONE = 0, ACT_LEAKY = 1, ACT_SILU = 2 };
enum Kind { CONV_IN, RES, DOWN, ATTN, UP };

struct Blk { Kind kind; std::string prefix; int cin, cout, sp; };
struct Plan {
    std::vector<std::vector<Blk>> in_blocks, out_blocks;
    std::vector<Blk> middle;
    int out_sp = 0;
};

struct Err : std::runtime_error { using std::runtime_error::runtime_error; };
[[noreturn]] void fail(const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    throw Err(buf);
}
void ok(int rc, const char* what) { if (rc != 0) fail("%s: %s", what, pixie_last_error()); }

bool has(const std::vector<int>& v, int x) { for (int e : v) if (e == x) return true; return false; }

struct Cfg {
    int feature_channels, cond_dim, model_channels, num_res_blocks;
    std::vector<int> mult, attn;
    int grid_size, out_channels, precision;
    bool has_projector() const { return feature_channels != cond_dim; }           // training_discrete.py:63-69
    int projector_hidden() const { return feature_channels > cond_dim ? 128 : 0; }  // 0: the light (1x1 + GroupNorm) projector
};

// diffusion_network.py:760-873, the constructor loop as data
Plan build_plan(const Cfg& c) {
    Plan p;
    const int mc = c.model_channels, nrb = c.num_res_blocks;
    auto name = [](const char* part, int idx, int sub) { return std::string("unet.") + part + "." + std::to_string(idx) + "." + std::to_string(sub); };
    p.in_blocks.push_back({Blk{CONV_IN, "unet.input_blocks.0.0", c.cond_dim, mc, c.grid_size}});
    std::vector<int> chans{mc}, sizes{c.grid_size};
    int ch = mc, ds = 1, sp = c.grid_size;
    for (size_t level = 0; level < c.mult.size(); ++level) {
        const int m = c.mult[level];
        for (int r = 0; r < nrb; ++r) {
            const int idx = (int)p.in_blocks.size();
            std::vector<Blk> seq{Blk{RES, name("input_blocks", idx, 0), ch, m * mc, sp}};
            ch = m * mc;
            if (has(c.attn, ds)) seq.push_back(Blk{ATTN, name("input_blocks", idx, 1), ch, ch, sp});
            p.in_blocks.push_back(seq);
            chans.push_back(ch);
        }
        if (level + 1 != c.mult.size()) {
            const int idx = (int)p.in_blocks.size();
            p.in_blocks.push_back({Blk{DOWN, name("input_blocks", idx, 0), ch, ch, sp}});
            chans.push_back(ch);
            sizes.push_back(sp);
            ds *= 2;
            sp = (sp + 1) / 2;
        }
    }
    p.middle = {Blk{RES, "unet.middle_block.0", ch, ch, sp}, Blk{ATTN, "unet.middle_block.1", ch, ch, sp}, Blk{RES, "unet.middle_block.2", ch, ch, sp}};
    for (int level = (int)c.mult.size() - 1; level >= 0; --level) {
        const int m = c.mult[level];
        for (int i = 0; i <= nrb; ++i) {
            const int idx = (int)p.out_blocks.size();
            const int ich = chans.back(); chans.pop_back();
            std::vector<Blk> seq{Blk{RES, name("output_blocks", idx, 0), ch + ich, mc * m, sp}};
            ch = mc * m;
            if (has(c.attn, ds)) seq.push_back(Blk{ATTN, name("output_blocks", idx, (int)seq.size()), ch, ch, sp});
            if (level && i == nrb) {
                seq.push_back(Blk{UP, name("output_blocks", idx, (int)seq.size()), ch, ch, sp});
                ds /= 2;
                sp = sizes.back(); sizes.pop_back();
            }
            p.out_blocks.push_back(seq);
        }
    }
    p.out_sp = sp;
    return p;
}

struct Param {
    std::string key;
    std::vector<int64_t> shape;
    int64_t numel = 1;
    bool norm = false;
    const float* d = nullptr;     // caller-owned device memory
    uint64_t version = 0;         // bumped by every pixie_unet_set_param
};

// state_dict keys and shapes in the reference's registration order
std::vector<Param> param_table(const Cfg& c, const Plan& plan) {
    std::vector<Param> out;
    auto add = [&](const std::string& key, std::vector<int64_t> shape, bool norm) {
        Param p; p.key = key; p.shape = shape; p.norm = norm;
        for (int64_t s : shape) p.numel *= s;
        out.push_back(p);
    };
    auto conv = [&](const std::string& prefix, int cout, int cin, int k, int dims = 3) {
        std::vector<int64_t> s{cout, cin};
        for (int i = 0; i < dims; ++i) s.push_back(k);
        add(prefix + ".weight", s, false);
        add(prefix + ".bias", {cout}, false);
    };
    auto norm = [&](const std::string& prefix, std::vector<int64_t> shape) {
        add(prefix + ".weight", shape, true);
        add(prefix + ".bias", shape, true);
    };
    if (c.has_projector()) {   // diffusion_network.py:556-585
        const int hid = c.projector_hidden();
        if (!hid) {
            conv("projector.net.0", c.cond_dim, c.feature_channels, 1);
            norm("projector.net.1", {c.cond_dim});
        } else {
            conv("projector.net.0", hid, c.feature_channels, 1);
            norm("projector.net.1", {hid});
            conv("projector.net.3", hid, hid, 3);
            norm("projector.net.4", {hid});
            conv("projector.net.6", c.cond_dim, hid, 1);
            norm("projector.net.7", {c.cond_dim});
        }
    }
    auto emit = [&](const Blk& b) {
        const std::vector<int64_t> vol{b.sp, b.sp, b.sp};
        switch (b.kind) {
            case CONV_IN: conv(b.prefix, b.cout, b.cin, 3); break;
            case RES:     // :673-694
                norm(b.prefix + ".in_layers.0", vol);
                conv(b.prefix + ".in_layers.2", b.cout, b.cin, 3);
                norm(b.prefix + ".out_layers.0", vol);
                conv(b.prefix + ".out_layers.3", b.cout, b.cout, 3);
                if (b.cin != b.cout) conv(b.prefix + ".skip_connection", b.cout, b.cin, 1);
                break;
            case DOWN: conv(b.prefix + ".op", b.cout, b.cin, 3); break;
            case UP:   conv(b.prefix + ".conv", b.cout, b.cin, 3); break;
            case ATTN:    // :199-208
                norm(b.prefix + ".norm", {b.cin});
                conv(b.prefix + ".qkv", 3 * b.cin, b.cin, 1, 1);
                conv(b.prefix + ".proj_out", b.cin, b.cin, 1, 1);
                break;
        }
    };
    for (auto& seq : plan.in_blocks) for (auto& b : seq) emit(b);
    for (auto& b : plan.middle) emit(b);
    for (auto& seq : plan.out_blocks) for (auto& b : seq) emit(b);
    norm("unet.out.0", {plan.out_sp, plan.out_sp, plan.out_sp});
    conv("unet.out.2", c.out_channels, c.model_channels, 3);
    return out;
}

// First-fit free list over [0, capacity) in units of bytes; 256-byte granules.  `base == nullptr` = dry run (offsets only).
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
    int64_t alloc(int64_t bytes) {
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
        fail("pixie_unet_forward: the workspace is too small (%lld bytes; ask pixie_unet_workspace_bytes for this grid size)", (long long)capacity);
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

struct Exec;
struct Tens {
    Exec* ex = nullptr;
    float* p = nullptr;
    int64_t off = -1;             // arena offset, -1: caller-owned
    int c = 0, d = 0, h = 0, w = 0;
    int64_t sums_off = -1;        // arena range of `sums` when a conv epilogue produced them (-1: pre-zeroed region, or none yet)
    bool has_sums = false;        // double[2c] channel sums of this tensor exist (somebody needed them)
    double* sums = nullptr;
    // the producing conv left partial statistics (pixie_conv_desc.d_out_stats) that nobody has added up yet: the first
    // normalisation that reads the tensor does, in the launch that also makes its affine (pixie_stats_norm_finalize)
    int64_t partials_off = -1;
    pixie_conv_desc pdesc;
    uint32_t* slot = nullptr;     // |x|max as float bits
    int64_t spatial() const { return (int64_t)d * h * w; }
    ~Tens();
};
using TP = std::shared_ptr<Tens>;

struct Packed { void* d = nullptr; uint64_t version = ~0ull; };
struct Sized { int64_t bytes; int slots; int64_t zsum_doubles; };   // workspace bytes, |x|max words, pre-zeroed statistics doubles
struct Bound { float wmax = 0, bmax = 0; uint64_t wver = ~0ull, bver = ~0ull; };

}  // namespace
}  // namespace pixie

using namespace pixie;

struct pixie_unet {
    Cfg cfg;
    Plan plan;
    std::vector<Param> params;
    std::unordered_map<std::string, int> index;
    std::unordered_map<std::string, Packed> packed32, packed16;
    std::unordered_map<std::string, Bound> bounds;
    uint32_t* d_bound_slots = nullptr;     // 2 words per normalisation layer, device
    std::vector<uint32_t> h_bound_slots;
    std::map<std::tuple<int, int, int, bool>, Sized> sized;   // (d, h, w, starts behind projector.net[0]) -> what one pass needs
    bool fuse_stats = true, split_k = true, fold_skip = true, subpixel = true;
    bool split_stats = true;               // split-K layers take their output's statistics in the reduce (PIXIE_SPLIT_STATS=0: a separate pass)
    // pixie_unet_set_option("graph", 1): forward() replays a captured HIP graph when called again with the same pointers
    struct Replay { const float* feat; const float* proj0; float* out; void* ws; int d; uint64_t epoch; hipGraph_t graph; hipGraphExec_t exec; };
    bool use_graph = false;
    uint64_t epoch = 0;                     // bumped by every set_param: captured kernel arguments (bounds, weights) are stale after it
    std::vector<Replay> replays;            // most recently used last; at most kMaxReplays
    static constexpr size_t kMaxReplays = 4;
    void drop_replay(size_t i) {
        (void)hipGraphExecDestroy(replays[i].exec);
        (void)hipGraphDestroy(replays[i].graph);
        replays.erase(replays.begin() + (long)i);
    }

    const Param& param(const std::string& key) const {
        auto it = index.find(key);
        if (it == index.end()) fail("pixie_unet: no parameter named '%s'", key.c_str());
        return params[it->second];
    }
};

namespace pixie {
namespace {

struct Exec {
    pixie_unet* net = nullptr;
    Arena arena;
    bool dry = false;
    void* stream = nullptr;
    // head of the workspace, zeroed by ONE memset per pass: |x|max words, then the double[2c] targets of the statistics passes
    uint32_t* slots = nullptr;
    int slot_next = 0, slot_cap = 0;
    double* zsums = nullptr;
    int64_t zsum_next = 0, zsum_cap = 0;
    // record mode (pixie_unet_forward_pair): the launch sites append to this list instead of launching (launch_record.h); the walk
    // marks the section.  Weight packing is no part of a pass and still launches.
    LaunchList* rec = nullptr;
    // the statistics pass over the caller's input: `in_ptr` is that tensor; what the pass left (in_sums, in_slot) can serve a second
    // network that reads the same tensor behind this one on the stream (share_sums, share_slot: set = take these, launch nothing)
    const float* in_ptr = nullptr;
    double* in_sums = nullptr; uint32_t* in_slot = nullptr;
    double* share_sums = nullptr; uint32_t* share_slot = nullptr;

    TP make(int c, int d, int h, int w) {
        auto t = std::make_shared<Tens>();
        t->ex = this; t->c = c; t->d = d; t->h = h; t->w = w;
        t->off = arena.alloc((int64_t)c * d * h * w * sizeof(float));
        t->p = arena.ptr<float>(t->off);
        return t;
    }
    TP external(const float* p, int c, int d, int h, int w) {
        auto t = std::make_shared<Tens>();
        t->ex = this; t->p = const_cast<float*>(p); t->c = c; t->d = d; t->h = h; t->w = w;
        return t;
    }
    uint32_t* new_slot() {
        if (!dry && slot_next >= slot_cap) fail("pixie_unet_forward: out of |x|max slots (internal sizing error)");
        return dry ? (slot_next++, nullptr) : slots + slot_next++;
    }
    struct Scratch {   // a temporary that must outlive the launches that use it only in stream order: freed at once
        Exec* ex; int64_t off;
        Scratch(Exec* e, int64_t bytes) : ex(e), off(e->arena.alloc(bytes)) {}
        ~Scratch() { ex->arena.release(off); }
        template <class T> T* as() const { return ex->arena.ptr<T>(off); }
    };

    // ---- parameters ----
    const float* P(const std::string& key) {
        const Param& p = net->param(key);
        if (!dry && !p.d) fail("pixie_unet_forward: parameter '%s' was never set", key.c_str());
        return p.d;
    }
    const void* w16(const std::string& key, bool subpixel = false) {     // f16 hi/lo packing (or its sub-pixel form), once per parameter version
        const Param& p = net->param(key + ".weight");
        if (dry) return nullptr;
        Packed& e = net->packed16[subpixel ? key + "#subpixel" : key];
        if (e.version != p.version) {
            const int cout = (int)p.shape[0], cin = (int)p.shape[1], k = (int)p.shape[2];
            const int64_t nb = subpixel ? (k == 3 ? pixie_conv_subpixel_bytes(cout, cin) : 0) : pixie_conv_packed16_bytes(cout, cin, k);
            if (nb <= 0) fail("pixie_unet: '%s' cannot take the f16x3 packing (c_in %d)", key.c_str(), cin);
            if (!e.d && hipMalloc(&e.d, (size_t)nb) != hipSuccess) fail("pixie_unet: hipMalloc of %lld bytes failed", (long long)nb);
            if (!p.d) fail("pixie_unet_forward: parameter '%s.weight' was never set", key.c_str());
            if (subpixel) ok(pixie_conv_pack_weights_subpixel(p.d, e.d, cout, cin, stream), "pixie_conv_pack_weights_subpixel");
            else ok(pixie_conv_pack_weights_f16x2(p.d, e.d, cout, cin, k, stream), "pixie_conv_pack_weights_f16x2");
            e.version = p.version;
        }
        return e.d;
    }
    const float* w32(const std::string& key) {    // [tap][c_in][c_out padded] fp32 packing
        const Param& p = net->param(key + ".weight");
        if (dry) return nullptr;
        Packed& e = net->packed32[key];
        if (e.version != p.version) {
            const int cout = (int)p.shape[0], cin = (int)p.shape[1], k = (int)p.shape[2];
            int64_t taps = 1;
            for (size_t i = 2; i < p.shape.size(); ++i) taps *= p.shape[i];
            const int64_t nb = taps * cin * pixie_conv_cout_padded(cout) * (int64_t)sizeof(float);
            if (!e.d && hipMalloc(&e.d, (size_t)nb) != hipSuccess) fail("pixie_unet: hipMalloc of %lld bytes failed", (long long)nb);
            if (!p.d) fail("pixie_unet_forward: parameter '%s.weight' was never set", key.c_str());
            ok(pixie_conv_pack_weights(p.d, static_cast<float*>(e.d), cout, cin, k, stream), "pixie_conv_pack_weights");
            e.version = p.version;
        }
        return static_cast<const float*>(e.d);
    }
    // Bound on |normalised * weight + bias| when `count` elements share the statistics: a standardised sample of n values
    // cannot exceed sqrt(n - 1) in magnitude; LeakyReLU / SiLU do not increase magnitudes.  (unet.py: _norm_bound)
    float norm_bound(const std::string& key, int64_t count) {
        if (dry) return 1.0f;
        const Bound& b = net->bounds[key];
        return (float)(std::sqrt((double)count) * (double)b.wmax + (double)b.bmax + 1e-30);
    }

    // ---- statistics ----
    void stats(const TP& t) {                  // channel sums + |x|max by a pass over the tensor (only where no conv produced them)
        if (t->has_sums || t->partials_off >= 0) return;
        t->has_sums = true;
        const bool input = t->off < 0 && in_ptr && t->p == in_ptr;
        if (input && share_slot) { t->sums = share_sums; t->slot = share_slot; return; }
        if (!dry && zsum_next + 2 * t->c > zsum_cap) fail("pixie_unet_forward: out of statistics space (internal sizing error)");
        t->sums = dry ? nullptr : zsums + zsum_next;      // the kernel adds into zeroed memory (fp64 atomics)
        zsum_next += 2 * t->c;
        t->slot = new_slot();
        if (!dry) ok(channel_stats_prezeroed(t->p, t->c, t->spatial(), t->sums, t->slot, as_stream(stream)), "pixie_channel_stats");
        if (input) { in_sums = t->sums; in_slot = t->slot; }
    }
    struct AB { std::shared_ptr<Scratch> mem; float* a; float* b; };
    // The prologue affine of a normalisation over th.cat(parts) (never materialised; statistics are read where they lie).
    // ONE launch: a part whose producer left partial statistics has them added up into its double[2c] sums here as well.
    AB norm_finalize(const std::vector<TP>& parts, int64_t spatial, int mode, int groups, const float* w, const float* b) {
        for (auto& t : parts) stats(t);
        const Tens* t0 = parts[0].get();
        const Tens* t1 = parts.size() > 1 ? parts[1].get() : nullptr;
        const int c0 = t0->c, c1 = t1 ? t1->c : 0, c = c0 + c1;
        AB r;
        const int cpad = (c + 63) / 64 * 64;
        r.mem = std::make_shared<Scratch>(this, (int64_t)(cpad + c) * sizeof(float));
        r.a = r.mem->as<float>();
        r.b = r.a + cpad;
        const bool p0 = t0->partials_off >= 0, p1 = t1 && t1->partials_off >= 0;
        if (p0 || p1) {
            // (part 0 carries the descriptor that tells its channel count even where its sums are final)
            pixie_conv_desc d0 = t0->pdesc;
            if (!p0) { std::memset(&d0, 0, sizeof d0); d0.c_out = c0; }
            if (!dry) ok(pixie_stats_norm_finalize(p0 ? arena.ptr<float>(t0->partials_off) : nullptr, &d0, t0->sums,
                                                   p1 ? arena.ptr<float>(t1->partials_off) : nullptr, p1 ? &t1->pdesc : nullptr, t1 ? t1->sums : nullptr,
                                                   c1, spatial, mode, groups, 1e-5, w, b, r.a, r.b, stream), "pixie_stats_norm_finalize");
            for (auto& t : parts)
                if (t->partials_off >= 0) { arena.release(t->partials_off); t->partials_off = -1; t->has_sums = true; }   // stream order: free at once
        } else if (!t1) {
            if (!dry) ok(pixie_norm_finalize(t0->sums, c, spatial, mode, groups, 1e-5, w, b, r.a, r.b, stream), "pixie_norm_finalize");
        } else {
            if (!dry) ok(norm_finalize_cat(t0->sums, c0, t1->sums, c1, spatial, mode, groups, 1e-5, w, b, r.a, r.b, as_stream(stream)), "pixie_norm_finalize");
        }
        return r;
    }

    // The plan of a launch over th.cat(parts): the f16x3 path where the network's precision asks for it and the shape allows it
    // (unet.py: HipOps.f16x3_ok), else exact fp32.  The caller sets the sub-pixel, crop and skip fields of s first.
    ConvPlan plan_conv(ConvShape& s, const std::vector<TP>& parts, int cout, int ksize, int stride, bool upsample) const {
        s.c0 = parts[0]->c; s.c1 = parts.size() > 1 ? parts[1]->c : 0; s.c_out = cout;
        s.in_d = parts[0]->d; s.in_h = parts[0]->h; s.in_w = parts[0]->w;
        s.ksize = ksize; s.stride = stride; s.upsample = upsample ? 1 : 0;
        s.w16 = net->cfg.precision == 0; s.workspace = net->split_k; s.exact_v1 = conv_exact_v1();
        ConvPlan p = conv_plan(s);
        if (p.refusal == CONV_BAD_CHANNELS) { s.w16 = s.subpixel = s.skip = false; p = conv_plan(s); }
        return p;
    }
    bool skip_foldable(const TP& x, int cout, int ksize, const std::vector<TP>& sp) const {   // unet.py: HipOps.skip_foldable
        ConvShape s;
        s.skip_c0 = sp[0]->c; s.skip_c1 = sp.size() > 1 ? sp[1]->c : 0;
        return plan_conv(s, {x}, cout, ksize, 1, false).skip_foldable;
    }

    // ---- one convolution launch (unet.py: UNetRunner._conv + HipOps.conv) ----
    struct ConvOpt {
        int stride = 1; bool upsample = false;
        const AB* pro = nullptr; std::string affine_store;     // affine_store: key of the spatial LayerNorm whose gamma/beta the prologue applies
        int act = ACT_NONE; TP residual; float bound = 0.0f;
        int out_d = 0, out_h = 0, out_w = 0;
        float* out_ptr = nullptr;                               // write the result here (caller-owned) instead of into the arena
        const std::vector<TP>* skip_parts = nullptr; std::string skip_key;   // folded 1x1x1 skip convolution over these raw tensors
    };
    TP conv(const std::vector<TP>& parts, const std::string& wkey, int cout, int ksize, const ConvOpt& o) {
        const TP& x0 = parts[0];
        const Tens* x1 = parts.size() > 1 ? parts[1].get() : nullptr;
        ConvShape s;
        s.out_d = o.out_d; s.out_h = o.out_h; s.out_w = o.out_w;   // odd-grid crop (diffusion_network.py:925-930): the cropped voxels are never computed
        s.subpixel = net->subpixel && o.upsample && ksize == 3 && o.stride == 1;   // unet.py: UNetRunner._conv
        if (o.skip_parts) { s.skip = true; s.skip_c0 = (*o.skip_parts)[0]->c; s.skip_c1 = o.skip_parts->size() > 1 ? (*o.skip_parts)[1]->c : 0; }
        const ConvPlan plan = plan_conv(s, parts, cout, ksize, o.stride, o.upsample);
        const int od = plan.OD, oh = plan.OH, ow = plan.OW;
        pixie_conv_desc desc;
        std::memset(&desc, 0, sizeof desc);
        if (o.out_d) { desc.out_d = od; desc.out_h = oh; desc.out_w = ow; }
        const bool f16 = s.w16;   // (a shape the f16x3 path refuses for another reason is pixie_conv3d_forward's to report)
        const bool raw = !o.pro && o.affine_store.empty();
        if (f16 && raw) for (auto& t : parts) stats(t);       // the input scale comes from the tensors' device-side |x|max

        TP out = o.out_ptr ? external(o.out_ptr, cout, od, oh, ow) : make(cout, od, oh, ow);
        desc.d_in0 = x0->p; desc.c0 = x0->c;
        desc.d_in1 = x1 ? x1->p : nullptr; desc.c1 = x1 ? x1->c : 0;
        desc.in_d = x0->d; desc.in_h = x0->h; desc.in_w = x0->w;
        desc.upsample = o.upsample ? 1 : 0;
        desc.stride = o.stride;
        desc.ksize = ksize;
        if (o.pro) { desc.d_pro_a = o.pro->a; desc.d_pro_b = o.pro->b; }
        if (!o.affine_store.empty()) { desc.d_gamma = P(o.affine_store + ".weight"); desc.d_beta = P(o.affine_store + ".bias"); }
        desc.act = o.act;
        desc.d_bias = P(wkey + ".bias");
        desc.c_out = cout;
        desc.d_residual = o.residual ? o.residual->p : nullptr;
        desc.d_out = out->p;
        if (!f16) {
            desc.d_w = w32(wkey);
            if (!dry) ok(pixie_conv3d_forward(&desc, stream), "pixie_conv3d_forward");
            return out;
        }
        desc.d_w16 = w16(wkey, s.subpixel);
        desc.w16_subpixel = s.subpixel ? 1 : 0;
        if (o.skip_parts) {
            const std::vector<TP>& sp = *o.skip_parts;
            desc.d_skip_in0 = sp[0]->p; desc.skip_c0 = sp[0]->c;
            desc.d_skip_in1 = sp.size() > 1 ? sp[1]->p : nullptr; desc.skip_c1 = sp.size() > 1 ? sp[1]->c : 0;
            desc.d_skip_w16 = w16(o.skip_key);
            desc.d_skip_bias = P(o.skip_key + ".bias");
            desc.d_skip_amax0 = sp[0]->slot; desc.d_skip_amax1 = sp.size() > 1 ? sp[1]->slot : nullptr;
        }
        if (raw) {
            desc.d_in_amax0 = parts[0]->slot;
            desc.d_in_amax1 = x1 ? parts[1]->slot : nullptr;
        } else {
            desc.in_bound = o.bound;
        }
        // the optional buffers are sized by the plan, which depends on the shape fields only: the dry run takes the same route
        std::unique_ptr<Scratch> workspace;
        if (plan.workspace_bytes > 0) { workspace.reset(new Scratch(this, plan.workspace_bytes)); desc.d_workspace = workspace->as<void>(); }
        bool have_stats = false;
        if (net->fuse_stats) {
            // the output's channel sums and |x|max come out of the conv epilogue: no separate pass over the tensor
            uint32_t* slot = new_slot();
            const int64_t nfl = plan.stats_floats;
            if (nfl > 0 && (!workspace || net->split_stats)) {   // (split-K layers too: their reduce takes the statistics)
                out->partials_off = arena.alloc(nfl * (int64_t)sizeof(float));
                desc.d_out_stats = arena.ptr<float>(out->partials_off);
                desc.d_out_amax = slot;
                have_stats = true;
                out->slot = slot;
            }
        }
        if (!dry) ok(pixie_conv3d_forward(&desc, stream), "pixie_conv3d_forward");
        if (have_stats) {   // the partials stay until a normalisation reads the tensor (norm_finalize); if none does, nothing adds them up
            out->sums_off = arena.alloc((int64_t)cout * 2 * sizeof(double));
            out->sums = arena.ptr<double>(out->sums_off);
            out->pdesc = desc;
        }
        return out;
    }

    // ---- blocks ----
    TP res(const Blk& b, const std::vector<TP>& parts) {   // MyResBlock.forward, diffusion_network.py:696-705
        const std::string& p = b.prefix;
        const int64_t spatial = parts[0]->spatial();
        AB pro = norm_finalize(parts, spatial, 0, 1, nullptr, nullptr);
        ConvOpt o1; o1.pro = &pro; o1.affine_store = p + ".in_layers.0"; o1.act = ACT_LEAKY; o1.bound = norm_bound(p + ".in_layers.0", spatial);
        TP h = conv(parts, p + ".in_layers.2", b.cout, 3, o1);
        AB pro2 = norm_finalize({h}, spatial, 0, 1, nullptr, nullptr);
        TP skip = parts[0];
        ConvOpt o2; o2.pro = &pro2; o2.affine_store = p + ".out_layers.0"; o2.act = ACT_LEAKY; o2.bound = norm_bound(p + ".out_layers.0", spatial);
        if (b.cin != b.cout) {
            if (net->fold_skip && skip_foldable(h, b.cout, 3, parts)) {
                // out = conv(h) + skip_connection(x) in ONE launch: the 1x1x1 convolution rides in the accumulators of the second
                // 3^3 convolution, the skip tensor never exists (conv16_skip.h, "folded skip")
                skip.reset();
                for (auto& t : parts) stats(t);
                o2.skip_parts = &parts; o2.skip_key = p + ".skip_connection";
            } else {
                skip = conv(parts, p + ".skip_connection", b.cout, 1, ConvOpt{});
            }
        }
        o2.residual = skip;
        return conv({h}, p + ".out_layers.3", b.cout, 3, o2);
    }
    TP attn(const Blk& b, const TP& x) {   // AttentionBlock._forward, diffusion_network.py:213-221
        const std::string& p = b.prefix;
        const int c = x->c;
        const int64_t spatial = x->spatial();
        AB pro = norm_finalize({x}, spatial, 1, 32, P(p + ".norm.weight"), P(p + ".norm.bias"));
        ConvOpt o; o.pro = &pro; o.bound = norm_bound(p + ".norm", spatial * (c / 32));
        TP qkv = conv({x}, p + ".qkv", 3 * c, 1, o);
        TP att = make(c, x->d, x->h, x->w);
        if (!dry) ok(pixie_attention_forward(qkv->p, att->p, c, (int)spatial, stream), "pixie_attention_forward");
        qkv.reset();
        ConvOpt o2; o2.residual = x;
        return conv({att}, p + ".proj_out", c, 1, o2);
    }
    TP block(const Blk& b, const std::vector<TP>& parts, const Tens* up_to) {
        if (b.kind == RES) return res(b, parts);
        const TP& x = parts[0];
        if (b.kind == ATTN) return attn(b, x);
        if (b.kind == DOWN) {
            if (rec && x->d == net->cfg.grid_size) rec->section = SEC_INNER;      // the inner section starts at the first stride-2 conv
            ConvOpt o; o.stride = 2; return conv({x}, b.prefix + ".op", b.cout, 3, o);
        }
        if (b.kind == UP) {
            // `up_to`: the skip tensor this output will be concatenated with; on odd grids it is one voxel smaller than
            // 2 * sp per axis and the reference crops h[..., :-1] (diffusion_network.py:925-930)
            ConvOpt o; o.upsample = true;
            if (up_to) { o.out_d = up_to->d; o.out_h = up_to->h; o.out_w = up_to->w; }
            if (rec && (up_to ? up_to->d : 2 * x->d) == net->cfg.grid_size) rec->section = SEC_FULLRES;   // ... and ends before the up-conv back to full resolution
            return conv({x}, b.prefix + ".conv", b.cout, 3, o);
        }
        fail("pixie_unet: unexpected block kind");
    }

    TP forward(const float* d_feat, const float* d_proj0, int D, int H, int W, float* d_out) {
        const Cfg& c = net->cfg;
        const int64_t spatial = (int64_t)D * H * W;
        TP x;
        AB pro_in; const AB* pro_in_p = nullptr;
        int act_in = ACT_NONE; float bound_in = 0.0f;
        if (c.has_projector()) {   // FeatureProjector.net, diffusion_network.py:556-585
            const std::string q = "projector.net.";
            const int hid = c.projector_hidden();
            if (!hid) {
                const int g = std::max(c.cond_dim / 2, 1);
                x = conv({external(d_feat, c.feature_channels, D, H, W)}, q + "0", c.cond_dim, 1, ConvOpt{});
                pro_in = norm_finalize({x}, spatial, 1, g, P(q + "1.weight"), P(q + "1.bias"));
                act_in = ACT_SILU;
                bound_in = norm_bound(q + "1", spatial * (c.cond_dim / g));
            } else {
                if (d_proj0) x = external(d_proj0, hid, D, H, W);
                else x = conv({external(d_feat, c.feature_channels, D, H, W)}, q + "0", hid, 1, ConvOpt{});
                AB pro = norm_finalize({x}, spatial, 1, 32, P(q + "1.weight"), P(q + "1.bias"));
                ConvOpt o; o.pro = &pro; o.act = ACT_SILU; o.bound = norm_bound(q + "1", spatial * (hid / 32));
                x = conv({x}, q + "3", hid, 3, o);
                AB pro2 = norm_finalize({x}, spatial, 1, 32, P(q + "4.weight"), P(q + "4.bias"));
                ConvOpt o2; o2.pro = &pro2; o2.act = ACT_SILU; o2.bound = norm_bound(q + "4", spatial * (hid / 32));
                x = conv({x}, q + "6", c.cond_dim, 1, o2);
                pro_in = norm_finalize({x}, spatial, 1, 32, P(q + "7.weight"), P(q + "7.bias"));
                bound_in = norm_bound(q + "7", spatial * std::max(c.cond_dim / 32, 1));
            }
            pro_in_p = &pro_in;
        } else {
            x = external(d_feat, c.feature_channels, D, H, W);
        }
        const Plan& plan = net->plan;
        std::vector<TP> hs;
        const Blk& first = plan.in_blocks[0][0];
        ConvOpt of; of.pro = pro_in_p; of.act = act_in; of.bound = bound_in;
        TP h = conv({x}, first.prefix, first.cout, 3, of);
        x.reset();
        pro_in = AB{};
        hs.push_back(h);
        for (size_t i = 1; i < plan.in_blocks.size(); ++i) {
            for (const Blk& b : plan.in_blocks[i]) h = block(b, {h}, nullptr);
            hs.push_back(h);
        }
        for (const Blk& b : plan.middle) h = block(b, {h}, nullptr);
        for (auto& seq : plan.out_blocks) {
            TP skip = hs.back(); hs.pop_back();
            if (skip->d != h->d || skip->h != h->h || skip->w != h->w) fail("pixie_unet_forward: skip tensor and decoder tensor differ in size");
            std::vector<TP> parts{h, skip};   // th.cat([h, hs.pop()], dim=1), :932 -- never materialised
            h.reset(); skip.reset();
            for (const Blk& b : seq) {
                TP nh = block(b, parts, (b.kind == UP && !hs.empty()) ? hs.back().get() : nullptr);
                parts.clear();
                parts.push_back(nh);
            }
            h = parts[0];
        }
        AB pro = norm_finalize({h}, h->spatial(), 0, 1, nullptr, nullptr);
        ConvOpt oo; oo.pro = &pro; oo.affine_store = "unet.out.0"; oo.act = ACT_LEAKY; oo.bound = norm_bound("unet.out.0", h->spatial());
        oo.out_ptr = d_out;
        return conv({h}, "unet.out.2", c.out_channels, 3, oo);
    }
};

Tens::~Tens() {
    if (!ex) return;
    if (off >= 0) ex->arena.release(off);
    if (sums_off >= 0) ex->arena.release(sums_off);
    if (partials_off >= 0) ex->arena.release(partials_off);
}

// max|weight| and max|bias| of every normalisation layer whose parameters changed: device reductions, ONE copy, ONE
// synchronisation (first pass after set_param only; a pass whose bounds are current never synchronises).
void refresh_bounds(pixie_unet* net, void* stream) {
    std::vector<std::pair<std::string, int>> todo;   // (layer key, word index)
    int n_norm = 0;
    for (const Param& p : net->params) {
        if (!p.norm || p.key.size() < 7 || p.key.compare(p.key.size() - 7, 7, ".weight") != 0) continue;
        const std::string key = p.key.substr(0, p.key.size() - 7);
        const Param& pb = net->param(key + ".bias");
        Bound& b = net->bounds[key];
        if (b.wver != p.version || b.bver != pb.version) todo.push_back({key, 2 * n_norm});
        ++n_norm;
    }
    if (todo.empty()) return;
    const size_t bytes = (size_t)2 * n_norm * sizeof(uint32_t);
    if (!net->d_bound_slots && hipMalloc(&net->d_bound_slots, bytes) != hipSuccess) fail("pixie_unet: hipMalloc failed");
    net->h_bound_slots.assign((size_t)2 * n_norm, 0u);
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(net->d_bound_slots, 0, bytes, s) != hipSuccess) fail("pixie_unet: hipMemsetAsync failed");
    for (auto& t : todo) {
        const Param& pw = net->param(t.first + ".weight");
        const Param& pb = net->param(t.first + ".bias");
        if (!pw.d || !pb.d) fail("pixie_unet_forward: parameter '%s' was never set", t.first.c_str());
        ok(pixie_tensor_amax(pw.d, pw.numel, net->d_bound_slots + t.second, stream), "pixie_tensor_amax");
        ok(pixie_tensor_amax(pb.d, pb.numel, net->d_bound_slots + t.second + 1, stream), "pixie_tensor_amax");
    }
    if (hipMemcpyAsync(net->h_bound_slots.data(), net->d_bound_slots, bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        fail("pixie_unet: reading the normalisation bounds back failed: %s", hipGetErrorString(hipGetLastError()));
    for (auto& t : todo) {
        Bound& b = net->bounds[t.first];
        std::memcpy(&b.wmax, &net->h_bound_slots[t.second], 4);
        std::memcpy(&b.bmax, &net->h_bound_slots[t.second + 1], 4);
        b.wver = net->param(t.first + ".weight").version;
        b.bver = net->param(t.first + ".bias").version;
    }
}

__global__ void zero_head_kernel(uint4* p, int64_t n16) {   // head_bytes is a multiple of kSlotAlign (256)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

constexpr int64_t kSlotAlign = 256;
int64_t slot_region_bytes(int n_slots) { return ((int64_t)n_slots * 4 + kSlotAlign - 1) / kSlotAlign * kSlotAlign; }
int64_t zsum_region_bytes(int64_t n_doubles) { return (n_doubles * 8 + kSlotAlign - 1) / kSlotAlign * kSlotAlign; }

Sized size_pass(pixie_unet* net, int D, int H, int W, bool from_proj0) {
    auto key = std::make_tuple(D, H, W, from_proj0);
    auto it = net->sized.find(key);
    if (it != net->sized.end()) return it->second;
    Exec ex;
    ex.net = net; ex.dry = true; ex.stream = nullptr;
    ex.arena.reset(reinterpret_cast<char*>(0x10000000), (int64_t)1 << 50);   // addresses of the dry run are never dereferenced
    {
        const float* fake = reinterpret_cast<const float*>(0x100);
        TP out = ex.forward(from_proj0 ? nullptr : fake, from_proj0 ? fake : nullptr, D, H, W, reinterpret_cast<float*>(0x100));
    }
    Sized r{ex.arena.peak + slot_region_bytes(ex.slot_next) + zsum_region_bytes(ex.zsum_next), ex.slot_next, ex.zsum_next};
    net->sized[key] = r;
    return r;
}

// One pass: the head of the workspace cleared, then the plan walk.  `rec`: append the launches to this list instead of launching
// them.  `share`: a pass over the same d_feat that goes out on the stream before this one; its input statistics are taken over.
void run_pass(pixie_unet* h, const float* d_feat, const float* d_proj0, int d, int hh, int w, float* d_out, void* d_workspace, int64_t workspace_bytes,
              const Sized& sized, void* stream, LaunchList* rec = nullptr, Exec* ex_out = nullptr, const Exec* share = nullptr) {
    Exec local;
    Exec& ex = ex_out ? *ex_out : local;
    ex.net = h; ex.dry = false; ex.stream = stream; ex.rec = rec;
    ex.in_ptr = d_feat;
    if (share && share->in_ptr == d_feat && share->in_slot) { ex.share_sums = share->in_sums; ex.share_slot = share->in_slot; }
    const int64_t slot_bytes = slot_region_bytes(sized.slots), head_bytes = slot_bytes + zsum_region_bytes(sized.zsum_doubles);
    ex.slots = static_cast<uint32_t*>(d_workspace);
    ex.slot_cap = sized.slots;
    ex.zsums = reinterpret_cast<double*>(static_cast<char*>(d_workspace) + slot_bytes);
    ex.zsum_cap = sized.zsum_doubles;
    struct Recording {   // the launch sites look at the calling thread's recorder
        LaunchList* before;
        explicit Recording(LaunchList* r) : before(launch_recorder()) { launch_recorder() = r; }
        ~Recording() { launch_recorder() = before; }
    } recording(rec);
    if (rec) rec->section = SEC_FULLRES;
    // Zeroed by a KERNEL, not hipMemsetAsync: as a node of a captured graph the memset did not reliably complete before
    // the kernels that follow it on ROCm 7.2 (replays of the f16x3 pass, whose first kernel already adds into this
    // region, gave wrong results at random once the workspace held a previous replay's values:
    // scripts/unet_soak.py, profiles/r3i_graph_replay_bisect.txt).  A kernel node has ordinary dependencies.
    px_launch(zero_head_kernel, dim3((unsigned)((head_bytes / 16 + 255) / 256)), dim3(256), 0, as_stream(stream),
              static_cast<uint4*>(d_workspace), head_bytes / 16);
    if (!rec && hipGetLastError() != hipSuccess) fail("pixie_unet_forward: clearing the workspace head failed");
    ex.arena.reset(static_cast<char*>(d_workspace) + head_bytes, workspace_bytes - head_bytes);
    TP out = ex.forward(d_feat, d_proj0, d, hh, w, d_out);
}

template <class F> int guarded(F f) {
    try { return f(); }
    catch (const std::exception& e) { return set_error("%s", e.what()); }
}

}  // namespace
}  // namespace pixie

extern "C" int pixie_unet_create(pixie_unet** out, const pixie_unet_config* c) {
    PX_REQUIRE(out && c, "pixie_unet_create: null argument");
    PX_REQUIRE(c->n_channel_mult >= 1 && c->n_channel_mult <= 8 && c->n_attention_resolutions >= 0 && c->n_attention_resolutions <= 8,
               "pixie_unet_create: channel_mult needs 1..8 entries, attention_resolutions 0..8");
    PX_REQUIRE(c->feature_channels > 0 && c->cond_dim > 0 && c->model_channels > 0 && c->num_res_blocks > 0 && c->grid_size > 0 && c->out_channels > 0,
               "pixie_unet_create: non-positive size");
    PX_REQUIRE(c->precision == 0 || c->precision == 1, "pixie_unet_create: precision is 0 (f16x3) or 1 (exact fp32)");
    return guarded([&] {
        std::unique_ptr<pixie_unet> n(new pixie_unet);
        n->cfg.feature_channels = c->feature_channels; n->cfg.cond_dim = c->cond_dim; n->cfg.model_channels = c->model_channels;
        n->cfg.num_res_blocks = c->num_res_blocks; n->cfg.grid_size = c->grid_size; n->cfg.out_channels = c->out_channels;
        n->cfg.precision = c->precision;
        n->cfg.mult.assign(c->channel_mult, c->channel_mult + c->n_channel_mult);
        n->cfg.attn.assign(c->attention_resolutions, c->attention_resolutions + c->n_attention_resolutions);
        n->plan = build_plan(n->cfg);
        n->params = param_table(n->cfg, n->plan);
        for (size_t i = 0; i < n->params.size(); ++i) n->index[n->params[i].key] = (int)i;
        const char* fs = getenv("PIXIE_FUSE_STATS"); n->fuse_stats = !(fs && fs[0] == '0');
        const char* sk = getenv("PIXIE_CONV_SPLIT_K"); n->split_k = !(sk && sk[0] == '0');
        const char* fk = getenv("PIXIE_FOLD_SKIP"); n->fold_skip = !(fk && fk[0] == '0');
        const char* ss = getenv("PIXIE_SPLIT_STATS"); n->split_stats = !(ss && ss[0] == '0');
        const char* sx = getenv("PIXIE_CONV_SUBPIXEL"); n->subpixel = !(sx && sx[0] == '0');
        *out = n.release();
        return 0;
    });
}

extern "C" int pixie_unet_destroy(pixie_unet* h) {
    if (!h) return 0;
    for (auto& kv : h->packed16) if (kv.second.d) (void)hipFree(kv.second.d);
    for (auto& kv : h->packed32) if (kv.second.d) (void)hipFree(kv.second.d);
    if (h->d_bound_slots) (void)hipFree(h->d_bound_slots);
    while (!h->replays.empty()) h->drop_replay(0);
    delete h;
    return 0;
}

extern "C" int pixie_unet_param_count(const pixie_unet* h) { return h ? (int)h->params.size() : 0; }

extern "C" int pixie_unet_param_info(const pixie_unet* h, int i, const char** key, int64_t* numel, int32_t* ndim, int64_t shape[5]) {
    PX_REQUIRE(h && i >= 0 && i < (int)h->params.size(), "pixie_unet_param_info: index out of range");
    const Param& p = h->params[i];
    if (key) *key = p.key.c_str();
    if (numel) *numel = p.numel;
    if (ndim) *ndim = (int32_t)p.shape.size();
    if (shape) for (size_t k = 0; k < p.shape.size() && k < 5; ++k) shape[k] = p.shape[k];
    return 0;
}

extern "C" int pixie_unet_set_param(pixie_unet* h, const char* key, const float* d_values, int64_t numel) {
    PX_REQUIRE(h && key && d_values, "pixie_unet_set_param: null argument");
    auto it = h->index.find(key);
    PX_REQUIRE(it != h->index.end(), "pixie_unet_set_param: unexpected key '%s' (the reference's load_state_dict(strict=True) raises here too)", key);
    Param& p = h->params[it->second];
    PX_REQUIRE(numel == p.numel, "pixie_unet_set_param: '%s' has %lld elements, got %lld", key, (long long)p.numel, (long long)numel);
    p.d = d_values;
    ++p.version;
    ++h->epoch;
    return 0;
}

extern "C" int64_t pixie_unet_workspace_bytes(pixie_unet* h, int d, int hh, int w) {
    if (!h || d <= 0 || hh <= 0 || w <= 0) { set_error("pixie_unet_workspace_bytes: bad argument"); return -1; }
    int64_t bytes = -1;
    const int rc = guarded([&] {   // enough for either entry: from the feature grid, or behind an externally computed projector.net[0]
        bytes = size_pass(h, d, hh, w, false).bytes;
        if (h->cfg.projector_hidden() > 0) bytes = std::max(bytes, size_pass(h, d, hh, w, true).bytes);
        return 0;
    });
    return rc == 0 ? bytes : -1;
}

extern "C" int pixie_unet_forward(pixie_unet* h, const float* d_feat, const float* d_proj0, int d, int hh, int w, float* d_out,
                                  void* d_workspace, int64_t workspace_bytes, void* stream) {
    PX_REQUIRE(h && d_out && d_workspace && (d_feat || d_proj0), "pixie_unet_forward: null argument");
    PX_REQUIRE(d == h->cfg.grid_size && hh == d && w == d,
               "pixie_unet_forward: the network was built for a %d^3 grid (its LayerNorm parameters have that shape), got %d x %d x %d", h->cfg.grid_size, d, hh, w);
    PX_REQUIRE(!d_proj0 || h->cfg.projector_hidden() > 0, "pixie_unet_forward: d_proj0 needs the hidden-128 projector (feature_channels > cond_dim)");
    PX_REQUIRE(d_feat || (d_proj0 && h->cfg.has_projector()), "pixie_unet_forward: d_feat is null");
    return guarded([&] {
        const auto sized = size_pass(h, d, hh, w, d_proj0 != nullptr);
        if (workspace_bytes < sized.bytes)
            fail("pixie_unet_forward: workspace of %lld bytes, this grid needs %lld (pixie_unet_workspace_bytes)", (long long)workspace_bytes, (long long)sized.bytes);
        auto launch_all = [&] { run_pass(h, d_feat, d_proj0, d, hh, w, d_out, d_workspace, workspace_bytes, sized, stream); };
        if (h->use_graph) {
            for (size_t i = 0; i < h->replays.size(); ++i) {
                const pixie_unet::Replay& r = h->replays[i];
                if (r.feat != d_feat || r.proj0 != d_proj0 || r.out != d_out || r.ws != d_workspace || r.d != d) continue;
                if (r.epoch != h->epoch) { h->drop_replay(i); break; }   // parameters changed since the capture
                if (hipGraphLaunch(r.exec, as_stream(stream)) != hipSuccess) fail("pixie_unet_forward: hipGraphLaunch failed: %s", hipGetErrorString(hipGetLastError()));
                if (i + 1 != h->replays.size()) std::rotate(h->replays.begin() + (long)i, h->replays.begin() + (long)i + 1, h->replays.end());
                return 0;
            }
        }
        // Recording needs a capturable stream: refuse BEFORE doing the work, so that the call either succeeds completely or
        // fails without having produced a result the caller would have to throw away.
        if (h->use_graph && as_stream(stream) == nullptr)
            fail("pixie_unet_forward: option \"graph\" needs a non-default stream (the legacy stream cannot be captured); pass a created stream or set graph = 0");
        refresh_bounds(h, stream);
        launch_all();               // eager: packs what needs packing, and IS this call's result
        if (h->use_graph) {
            // the same launch sequence once more, recorded instead of executed, for the next call with these pointers
            hipStream_t st = as_stream(stream);
            if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess)
                fail("pixie_unet_forward: cannot capture on this stream (graph replay needs a non-default stream): %s", hipGetErrorString(hipGetLastError()));
            hipGraph_t graph = nullptr;
            try { launch_all(); }
            catch (...) { (void)hipStreamEndCapture(st, &graph); if (graph) (void)hipGraphDestroy(graph); throw; }
            if (hipStreamEndCapture(st, &graph) != hipSuccess || !graph) fail("pixie_unet_forward: hipStreamEndCapture failed: %s", hipGetErrorString(hipGetLastError()));
            hipGraphExec_t exec = nullptr;
            if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) { (void)hipGraphDestroy(graph); fail("pixie_unet_forward: hipGraphInstantiate failed"); }
            if (h->replays.size() >= pixie_unet::kMaxReplays) h->drop_replay(0);
            h->replays.push_back(pixie_unet::Replay{d_feat, d_proj0, d_out, d_workspace, d, h->epoch, graph, exec});
        }
        return 0;
    });
}

extern "C" int pixie_unet_forward_pair(pixie_unet* h0, pixie_unet* h1, const float* d_feat, int d, int hh, int w, float* d_out0, float* d_out1,
                                       void* d_workspace0, int64_t workspace0_bytes, void* d_workspace1, int64_t workspace1_bytes, void* stream,
                                       int32_t* launch_counts) {
    PX_REQUIRE(h0 && h1 && h0 != h1 && d_feat && d_out0 && d_out1 && d_workspace0 && d_workspace1, "pixie_unet_forward_pair: null argument, or one handle twice");
    PX_REQUIRE(d_out0 != d_out1 && d_workspace0 != d_workspace1, "pixie_unet_forward_pair: the two networks need outputs and workspaces of their own");
    pixie_unet* hs[2] = {h0, h1};
    for (pixie_unet* h : hs)
        PX_REQUIRE(d == h->cfg.grid_size && hh == d && w == d,
                   "pixie_unet_forward_pair: a network was built for a %d^3 grid (its LayerNorm parameters have that shape), got %d x %d x %d", h->cfg.grid_size, d, hh, w);
    return guarded([&] {
        float* outs[2] = {d_out0, d_out1};
        void* wss[2] = {d_workspace0, d_workspace1};
        const int64_t wsb[2] = {workspace0_bytes, workspace1_bytes};
        Sized sized[2];
        for (int k = 0; k < 2; ++k) {
            sized[k] = size_pass(hs[k], d, hh, w, false);
            if (wsb[k] < sized[k].bytes)
                fail("pixie_unet_forward_pair: workspace %d of %lld bytes, this grid needs %lld (pixie_unet_workspace_bytes)", k, (long long)wsb[k], (long long)sized[k].bytes);
        }
        for (pixie_unet* h : hs) refresh_bounds(h, stream);
        // both walks in record mode (they pack what needs packing, on the stream, ahead of every launch of the pass) ...
        LaunchList lists[2];
        Exec ex[2];
        for (int k = 0; k < 2; ++k)
            run_pass(hs[k], d_feat, nullptr, d, hh, w, outs[k], wss[k], wsb[k], sized[k], stream, &lists[k], &ex[k], k ? &ex[0] : nullptr);
        // ... then one stream of launches: the levels below full resolution go out zipped, grouped where the two match
        int grouped = 0;
        const char* pg = getenv("PIXIE_UNET_PAIR_GROUP");
        const std::vector<LaunchRec> merged = merge_pair(lists[0], lists[1], &grouped, !(pg && pg[0] == '0'));
        for (const LaunchRec& r : merged)
            if (launch_rec(r, as_stream(stream)) != hipSuccess) fail("pixie_unet_forward_pair: a launch failed: %s", hipGetErrorString(hipGetLastError()));
        if (launch_counts) {
            launch_counts[0] = (int32_t)(lists[0].recs.size() + lists[1].recs.size()); launch_counts[1] = (int32_t)merged.size(); launch_counts[2] = grouped;
            launch_counts[3] = 0;
            for (const LaunchRec& r : merged) launch_counts[3] += r.net < 0 && r.lds > 0;   // of the small kernels none asks for dynamic LDS
        }
        return 0;
    });
}

extern "C" int pixie_unet_set_option(pixie_unet* h, const char* key, int value) {
    PX_REQUIRE(h && key, "pixie_unet_set_option: null argument");
    const std::string k(key);
    if (k == "graph") {
        h->use_graph = value != 0;
        if (!h->use_graph) while (!h->replays.empty()) h->drop_replay(0);
        return 0;
    }
    return set_error("pixie_unet_set_option: unknown key '%s' (known: graph)", key);
}
