// pixie_amd/csrc/unet_walk.h -- the plan walk of one U-Net pass: tensor lifetimes, statistics bookkeeping, the filling of every
// pixie_conv_desc, the blocks and forward().  The sizing run (dry: offsets only, nothing launched) and the real pass share this
// walk, so they take the same placement decisions; in record mode (pixie_unet_forward_pair) the launch sites append to a list
// instead of launching.  The launch order equals pixie_amd/unet.py: UNetRunner.forward, so both executors produce bit-identical
// tensors (tests/test_unet_hip.py).  The workspace placement is a function of the order of the alloc / release calls in here:
// tests/test_unet_handle.py pins pixie_unet_workspace_bytes, which moves when that order does.
//
// Net is what the walk reads and caches of a handle (unet_exec.hip: struct pixie_unet adds what only the entry points use).
#pragma once
#include <cmath>
#include <memory>
#include <stdexcept>
#include <unordered_map>

#include "common.h"
#include "conv_launch.h"
#include "launch_record.h"
#include "unet_ops_internal.h"
#include "unet_plan.h"
#include "workspace_arena.h"

namespace pixie::unet {

enum { ACT_NONE = 0, ACT_LEAKY = 1, ACT_SILU = 2 };

[[noreturn]] inline void fail(const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    throw std::runtime_error(buf);
}
inline void ok(int rc, const char* what) { if (rc != 0) fail("%s: %s", what, pixie_last_error()); }

struct Param : ParamSpec {
    const float* d = nullptr;     // caller-owned device memory
    uint64_t version = 0;         // bumped by every pixie_unet_set_param
};
struct Packed { void* d = nullptr; uint64_t version = ~0ull; };
struct Bound { float wmax = 0, bmax = 0; uint64_t wver = ~0ull, bver = ~0ull; };

struct Net {
    Cfg cfg;
    Plan plan;
    std::vector<Param> params;
    std::unordered_map<std::string, int> index;
    std::unordered_map<std::string, Packed> packed32, packed16;
    std::unordered_map<std::string, Bound> bounds;
    bool fuse_stats = true, split_k = true, fold_skip = true, subpixel = true;
    bool split_stats = true;               // split-K layers take their output's statistics in the reduce (PIXIE_SPLIT_STATS=0: a separate pass)

    const Param& param(const std::string& key) const {
        auto it = index.find(key);
        if (it == index.end()) fail("pixie_unet: no parameter named '%s'", key.c_str());
        return params[it->second];
    }
};

struct Tens {
    Arena* arena = nullptr;       // where off, sums_off and partials_off lie; they return there with the tensor
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
    ~Tens() {
        for (int64_t range : {off, sums_off, partials_off}) if (range >= 0) arena->release(range);
    }
};
using TP = std::shared_ptr<Tens>;

struct Exec {
    Net* net = nullptr;
    Arena arena;
    bool dry = false;
    void* stream = nullptr;
    // head of the workspace, zeroed by ONE launch per pass: |x|max words, then the double[2c] targets of the statistics passes
    uint32_t* slots = nullptr;
    int slot_next = 0, slot_cap = 0;
    double* zsums = nullptr;
    int64_t zsum_next = 0, zsum_cap = 0;
    // record mode (pixie_unet_forward_pair): the launch sites append to this list instead of launching (launch_record.h); the walk
    // marks the section.  Weight packing is no part of a pass and still launches.
    LaunchList* rec = nullptr;
    // the statistics pass over the caller's input: `in_ptr` is that tensor; what the pass left (in_sums, in_slot) can serve a second
    // network that reads the same tensor behind this one on the stream (`share`: that earlier pass; take its, launch nothing)
    const float* in_ptr = nullptr;
    double* in_sums = nullptr; uint32_t* in_slot = nullptr;
    const Exec* share = nullptr;

    int64_t alloc(int64_t bytes) {
        const int64_t off = arena.alloc(bytes);
        if (off < 0) fail("pixie_unet_forward: the workspace is too small (%lld bytes; ask pixie_unet_workspace_bytes for this grid size)", (long long)arena.capacity);
        return off;
    }
    TP external(const float* p, int c, int d, int h, int w) {
        auto t = std::make_shared<Tens>();
        t->arena = &arena; t->p = const_cast<float*>(p); t->c = c; t->d = d; t->h = h; t->w = w;
        return t;
    }
    TP make(int c, int d, int h, int w) {
        TP t = external(nullptr, c, d, h, w);
        t->off = alloc((int64_t)c * d * h * w * sizeof(float));
        t->p = arena.ptr<float>(t->off);
        return t;
    }
    uint32_t* new_slot() {
        if (!dry && slot_next >= slot_cap) fail("pixie_unet_forward: out of |x|max slots (internal sizing error)");
        return dry ? (slot_next++, nullptr) : slots + slot_next++;
    }

    // ---- parameters ----
    const float* P(const std::string& key) {
        const Param& p = net->param(key);
        if (!dry && !p.d) fail("pixie_unet_forward: parameter '%s' was never set", key.c_str());
        return p.d;
    }
    // The packed form of `key`.weight, made once per parameter version: [tap][c_in][c_out padded] fp32, the f16 hi/lo packing, or
    // that packing's sub-pixel form (cached beside it as `key`#subpixel).
    enum Packing { PACK_F32, PACK_F16, PACK_SUBPIXEL };
    const void* packed(const std::string& key, Packing kind) {
        const Param& p = net->param(key + ".weight");
        if (dry) return nullptr;
        Packed& e = kind == PACK_F32 ? net->packed32[key] : net->packed16[kind == PACK_SUBPIXEL ? key + "#subpixel" : key];
        if (e.version != p.version) {
            const int cout = (int)p.shape[0], cin = (int)p.shape[1], k = (int)p.shape[2];
            const int64_t nb = kind == PACK_F32 ? p.numel / cout * pixie_conv_cout_padded(cout) * (int64_t)sizeof(float)   // taps * c_in rows
                               : kind == PACK_F16 ? pixie_conv_packed16_bytes(cout, cin, k) : (k == 3 ? pixie_conv_subpixel_bytes(cout, cin) : 0);
            if (kind != PACK_F32 && nb <= 0) fail("pixie_unet: '%s' cannot take the f16x3 packing (c_in %d)", key.c_str(), cin);
            if (!e.d && hipMalloc(&e.d, (size_t)nb) != hipSuccess) fail("pixie_unet: hipMalloc of %lld bytes failed", (long long)nb);
            if (!p.d) fail("pixie_unet_forward: parameter '%s.weight' was never set", key.c_str());
            if (kind == PACK_F32) ok(pixie_conv_pack_weights(p.d, static_cast<float*>(e.d), cout, cin, k, stream), "pixie_conv_pack_weights");
            else if (kind == PACK_F16) ok(pixie_conv_pack_weights_f16x2(p.d, e.d, cout, cin, k, stream), "pixie_conv_pack_weights_f16x2");
            else ok(pixie_conv_pack_weights_subpixel(p.d, e.d, cout, cin, stream), "pixie_conv_pack_weights_subpixel");
            e.version = p.version;
        }
        return e.d;
    }
    // Bound on |normalised * weight + bias| when `count` elements share the statistics: a standardised sample of n values
    // cannot exceed sqrt(n - 1) in magnitude; LeakyReLU / SiLU do not increase magnitudes.  (unet.py: _norm_bound)
    float norm_bound(const std::string& key, int64_t count) {   // (the dry run computes it from zeroes; nothing reads it there)
        const Bound& b = net->bounds[key];
        return (float)(std::sqrt((double)count) * (double)b.wmax + (double)b.bmax + 1e-30);
    }

    // ---- statistics ----
    void stats(const TP& t) {                  // channel sums + |x|max by a pass over the tensor (only where no conv produced them)
        if (t->has_sums || t->partials_off >= 0) return;
        t->has_sums = true;
        const bool input = t->off < 0 && in_ptr && t->p == in_ptr;
        if (input && share && share->in_ptr == in_ptr && share->in_slot) { t->sums = share->in_sums; t->slot = share->in_slot; return; }
        if (!dry && zsum_next + 2 * t->c > zsum_cap) fail("pixie_unet_forward: out of statistics space (internal sizing error)");
        t->sums = dry ? nullptr : zsums + zsum_next;      // the kernel adds into zeroed memory (fp64 atomics)
        zsum_next += 2 * t->c;
        t->slot = new_slot();
        if (!dry) ok(channel_stats_prezeroed(t->p, t->c, t->spatial(), t->sums, t->slot, as_stream(stream)), "pixie_channel_stats");
        if (input) { in_sums = t->sums; in_slot = t->slot; }
    }
    struct AB { TP mem; float* a; float* b; };   // mem must outlive the launches that use it only in stream order: freed at once
    // The prologue affine of a normalisation over th.cat(parts) (never materialised; statistics are read where they lie).
    // ONE launch: a part whose producer left partial statistics has them added up into its double[2c] sums here as well.
    AB norm_finalize(const std::vector<TP>& parts, int64_t spatial, int mode, int groups, const float* w, const float* b) {
        for (auto& t : parts) stats(t);
        const Tens* t0 = parts[0].get();
        const Tens* t1 = parts.size() > 1 ? parts[1].get() : nullptr;
        const int c0 = t0->c, c1 = t1 ? t1->c : 0, c = c0 + c1;
        AB r;
        const int cpad = (c + 63) / 64 * 64;
        r.mem = make(cpad + c, 1, 1, 1);
        r.a = r.mem->p;
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

    // ---- one convolution launch (unet.py: UNetRunner._conv + HipOps.conv) ----
    struct ConvOpt {
        int stride = 1; bool upsample = false;
        const AB* pro = nullptr; std::string affine_store;     // affine_store: key of the spatial LayerNorm whose gamma/beta the prologue applies
        int act = ACT_NONE; TP residual; float bound = 0.0f;
        int out_d = 0, out_h = 0, out_w = 0;
        float* out_ptr = nullptr;                               // write the result here (caller-owned) instead of into the arena
        const std::vector<TP>* skip_parts = nullptr; std::string skip_key;   // folded 1x1x1 skip convolution over these raw tensors
    };
    // the options of a convolution behind the normalisation layer `key`, whose affine is `pro` and whose statistics `count` elements
    // share; `store`: the layer is a spatial LayerNorm, the prologue applies its stored gamma/beta as well
    ConvOpt behind_norm(const AB& pro, const std::string& key, int64_t count, int act, bool store) {
        ConvOpt o; o.pro = &pro; o.act = act; o.bound = norm_bound(key, count);
        if (store) o.affine_store = key;
        return o;
    }
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
            desc.d_w = static_cast<const float*>(packed(wkey, PACK_F32));
            if (!dry) ok(pixie_conv3d_forward(&desc, stream), "pixie_conv3d_forward");
            return out;
        }
        desc.d_w16 = packed(wkey, s.subpixel ? PACK_SUBPIXEL : PACK_F16);
        desc.w16_subpixel = s.subpixel ? 1 : 0;
        if (o.skip_parts) {
            const std::vector<TP>& sp = *o.skip_parts;
            desc.d_skip_in0 = sp[0]->p; desc.skip_c0 = sp[0]->c;
            desc.d_skip_in1 = sp.size() > 1 ? sp[1]->p : nullptr; desc.skip_c1 = sp.size() > 1 ? sp[1]->c : 0;
            desc.d_skip_w16 = packed(o.skip_key, PACK_F16);
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
        TP workspace;      // split-K: the slices' partial outputs, plan.workspace_bytes in all; needed only until the reduce is launched
        if (plan.workspace_bytes > 0) { workspace = make(plan.slices * cout, od, oh, ow); desc.d_workspace = workspace->p; }
        bool have_stats = false;
        if (net->fuse_stats) {
            // the output's channel sums and |x|max come out of the conv epilogue: no separate pass over the tensor
            uint32_t* slot = new_slot();
            const int64_t nfl = plan.stats_floats;
            if (nfl > 0 && (!workspace || net->split_stats)) {   // (split-K layers too: their reduce takes the statistics)
                out->partials_off = alloc(nfl * (int64_t)sizeof(float));
                desc.d_out_stats = arena.ptr<float>(out->partials_off);
                desc.d_out_amax = slot;
                have_stats = true;
                out->slot = slot;
            }
        }
        if (!dry) ok(pixie_conv3d_forward(&desc, stream), "pixie_conv3d_forward");
        if (have_stats) {   // the partials stay until a normalisation reads the tensor (norm_finalize); if none does, nothing adds them up
            out->sums_off = alloc((int64_t)cout * 2 * sizeof(double));
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
        TP h = conv(parts, p + ".in_layers.2", b.cout, 3, behind_norm(pro, p + ".in_layers.0", spatial, ACT_LEAKY, true));
        AB pro2 = norm_finalize({h}, spatial, 0, 1, nullptr, nullptr);
        TP skip = parts[0];
        ConvOpt o2 = behind_norm(pro2, p + ".out_layers.0", spatial, ACT_LEAKY, true);
        if (b.cin != b.cout) {
            ConvShape fs;      // the second 3^3 convolution with the skip's channels: unet.py: HipOps.skip_foldable
            fs.skip_c0 = parts[0]->c; fs.skip_c1 = parts.size() > 1 ? parts[1]->c : 0;
            if (net->fold_skip && plan_conv(fs, {h}, b.cout, 3, 1, false).skip_foldable) {
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
        TP qkv = conv({x}, p + ".qkv", 3 * c, 1, behind_norm(pro, p + ".norm", spatial * (c / 32), ACT_NONE, false));
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
        AB pro_in;
        ConvOpt of;                // of the first convolution of the U-Net proper: behind the projector's last normalisation, if there is one
        if (c.has_projector()) {   // FeatureProjector.net, diffusion_network.py:556-585
            const std::string q = "projector.net.";
            const int hid = c.projector_hidden();
            if (!hid) {
                const int g = std::max(c.cond_dim / 2, 1);
                x = conv({external(d_feat, c.feature_channels, D, H, W)}, q + "0", c.cond_dim, 1, ConvOpt{});
                pro_in = norm_finalize({x}, spatial, 1, g, P(q + "1.weight"), P(q + "1.bias"));
                of = behind_norm(pro_in, q + "1", spatial * (c.cond_dim / g), ACT_SILU, false);
            } else {
                if (d_proj0) x = external(d_proj0, hid, D, H, W);
                else x = conv({external(d_feat, c.feature_channels, D, H, W)}, q + "0", hid, 1, ConvOpt{});
                AB pro = norm_finalize({x}, spatial, 1, 32, P(q + "1.weight"), P(q + "1.bias"));
                x = conv({x}, q + "3", hid, 3, behind_norm(pro, q + "1", spatial * (hid / 32), ACT_SILU, false));
                AB pro2 = norm_finalize({x}, spatial, 1, 32, P(q + "4.weight"), P(q + "4.bias"));
                x = conv({x}, q + "6", c.cond_dim, 1, behind_norm(pro2, q + "4", spatial * (hid / 32), ACT_SILU, false));
                pro_in = norm_finalize({x}, spatial, 1, 32, P(q + "7.weight"), P(q + "7.bias"));
                of = behind_norm(pro_in, q + "7", spatial * std::max(c.cond_dim / 32, 1), ACT_NONE, false);
            }
        } else {
            x = external(d_feat, c.feature_channels, D, H, W);
        }
        std::vector<TP> hs;
        const Blk& first = net->plan.in_blocks[0][0];
        TP h = conv({x}, first.prefix, first.cout, 3, of);
        x.reset();
        pro_in = AB{};
        hs.push_back(h);
        for (size_t i = 1; i < net->plan.in_blocks.size(); ++i) {
            for (const Blk& b : net->plan.in_blocks[i]) h = block(b, {h}, nullptr);
            hs.push_back(h);
        }
        for (const Blk& b : net->plan.middle) h = block(b, {h}, nullptr);
        for (auto& seq : net->plan.out_blocks) {
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
        ConvOpt oo = behind_norm(pro, "unet.out.0", h->spatial(), ACT_LEAKY, true);
        oo.out_ptr = d_out;
        return conv({h}, "unet.out.2", c.out_channels, 3, oo);
    }
};

}  // namespace pixie::unet
