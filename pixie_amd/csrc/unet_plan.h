// pixie_amd/csrc/unet_plan.h -- the reference U-Net as data: the configuration, the block lists of MyUNetModel's constructor and the
// state_dict table (keys, shapes, which entries belong to a normalisation) in the reference's registration order.  Pure functions
// of the configuration with no HIP in them: unet_exec.hip builds a handle's plan and parameter table from them, unet_walk.h walks
// the plan, and tests/test_unet_host.py compiles this header alone with g++ under ASan/UBSan and holds it to
// pixie_amd/unet_plan.py (build_plan, param_shapes, is_norm_key) over a sweep of configurations.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace pixie::unet {

enum Kind { CONV_IN, RES, DOWN, ATTN, UP };

struct Blk { Kind kind; std::string prefix; int cin, cout, sp; };
struct Plan {
    std::vector<std::vector<Blk>> in_blocks, out_blocks;
    std::vector<Blk> middle;
    int out_sp = 0;
};

inline bool has(const std::vector<int>& v, int x) { for (int e : v) if (e == x) return true; return false; }

struct Cfg {
    int feature_channels, cond_dim, model_channels, num_res_blocks;
    std::vector<int> mult, attn;
    int grid_size, out_channels, precision;
    bool has_projector() const { return feature_channels != cond_dim; }           // training_discrete.py:63-69
    int projector_hidden() const { return feature_channels > cond_dim ? 128 : 0; }  // 0: the light (1x1 + GroupNorm) projector
};

// diffusion_network.py:760-873, the constructor loop as data
inline Plan build_plan(const Cfg& c) {
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

// one state_dict entry; the handle's Param (unet_walk.h) adds the caller's device pointer and its version
struct ParamSpec {
    std::string key;
    std::vector<int64_t> shape;
    int64_t numel = 1;
    bool norm = false;
};

// state_dict keys and shapes in the reference's registration order
template <class Entry = ParamSpec> std::vector<Entry> param_table(const Cfg& c, const Plan& plan) {
    std::vector<Entry> out;
    auto add = [&](const std::string& key, std::vector<int64_t> shape, bool norm) {
        Entry p; p.key = key; p.shape = shape; p.norm = norm;
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

}  // namespace pixie::unet
