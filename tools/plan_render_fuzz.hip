// Stand-alone host program: the render planner (plan_render through sn_rm_render_route_info, and sn_rm_render_workspace_bytes) over
// randomised cfg / io within the ABI's limits, for a sanitizer build.  Nothing is launched; no GPU is needed.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -ffp-contract=off -Wno-pass-failed -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/plan_render_fuzz.hip sanerf-hq_amd/csrc/grid.hip -o plan_render_fuzz
//   ./plan_render_fuzz 5000
// render.hip is compiled INTO this program and grid.hip beside it (set_error, build_grid_levels): every host function the planner runs
// is a sanitized copy, and the library is not linked.  The planner is entered through its two public doors: sn_rm_render_route_info
// (= check_io_pointers + plan_render) and sn_rm_render_workspace_bytes (= plan_workspace).
#include "../sanerf-hq_amd/csrc/render.hip"

#include <cmath>
#include <random>

static std::mt19937 rng(12345);
static uint32_t U(uint32_t lo, uint32_t hi) { return lo + rng() % (hi - lo + 1); }
static bool coin(int one_in) { return rng() % one_in == 0; }
static void *P() { return reinterpret_cast<void *>(64); }

static void grid(sn_grid_desc *d, uint32_t L, uint32_t C, uint32_t log2T, float desired, bool wild) {
    memset(d, 0, sizeof(*d));
    const double scale = L > 1 ? exp2(log2(desired / 16.0) / (L - 1)) : 1.0;
    int32_t off = 0;
    for (uint32_t l = 0; l < L; ++l) {
        const double res = ceil(16.0 * pow(scale, l));
        double rows = res * res * res;
        if (rows > (double)(1u << log2T)) rows = (double)(1u << log2T);
        d->offsets[l] = off;
        off += (int32_t)(ceil(rows / 8.0) * 8.0);
        if (wild && coin(8)) off += 8 * (int32_t)U(0, 5);
    }
    d->offsets[L] = off;
    d->embeddings = coin(20) ? nullptr : P();
    d->table_dtype = coin(2) ? SN_F16 : SN_F32;
    d->D = wild && coin(10) ? U(2, 5) : 3; d->C = C; d->L = L; d->S = (float)log2(scale); d->H = 16;
    d->gridtype = wild && coin(10) ? 1 : 0; d->align_corners = wild && coin(10); d->interp = wild && coin(10);
}
static void mlp(sn_mlp_desc *m, std::initializer_list<uint32_t> dims, bool wild) {
    memset(m, 0, sizeof(*m));
    m->num_layers = (uint32_t)dims.size() - 1;
    uint32_t i = 0;
    for (uint32_t v : dims) m->dims[i++] = v;
    if (wild) {
        m->num_layers = U(0, SN_MAX_LAYERS);
        for (uint32_t l = 0; l <= m->num_layers; ++l) m->dims[l] = coin(3) ? U(0, 80) : m->dims[l] ? m->dims[l] : U(1, 64);
    }
    for (uint32_t l = 0; l < m->num_layers; ++l) { m->weight[l] = coin(30) ? nullptr : (const float *)P(); m->bias[l] = coin(30) ? (const float *)P() : nullptr; }
    m->activation = coin(30); m->skip_mask = coin(30);
}

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 4000;
    int ok = 0, fail = 0;
    for (int it = 0; it < iters; ++it) {
        sn_render_cfg cfg;
        sn_render_io io;
        memset(&cfg, 0, sizeof(cfg));
        memset(&io, 0, sizeof(io));
        const bool wild = coin(3);
        cfg.num_stages = coin(25) ? U(0, SN_MAX_STAGES + 1) : U(1, SN_MAX_STAGES);
        for (uint32_t k = 0; k < SN_MAX_STAGES; ++k) cfg.num_steps[k] = coin(30) ? 0 : U(1, coin(4) ? 600 : 130);
        for (uint32_t k = 0; k < SN_MAX_STAGES; ++k) {
            grid(&cfg.prop_grid[k], wild && coin(6) ? U(1, SN_MAX_LEVELS) : 5, wild && coin(8) ? 4 : 2, 17, k ? 256.0f : 128.0f, wild);
            if (wild && coin(4)) mlp(&cfg.prop_mlp[k], {10, 16, 1}, true); else mlp(&cfg.prop_mlp[k], {10, 16, 1}, false);
        }
        const bool any = coin(4);
        const uint32_t L = any ? U(1, SN_MAX_LEVELS) : 16;
        grid(&cfg.grid, L, wild && coin(8) ? U(1, 8) : 2, U(10, 22), coin(2) ? 4096.0f : 512.0f, wild);
        if (any && !wild) { mlp(&cfg.grid_mlp, {L * 2, 32, 16}, false); mlp(&cfg.view_mlp, {31, 32, 3}, false); }
        else { mlp(&cfg.grid_mlp, {32, 64, 64, 16}, wild && coin(3)); mlp(&cfg.view_mlp, {31, 32, 32, 3}, wild && coin(3)); }
        cfg.sh_degree = coin(30) ? 3 : 4;
        cfg.bound = 2.0f; cfg.min_near = 0.2f;
        cfg.with_feat = coin(4);
        grid(&cfg.feat_grid, coin(3) ? U(1, SN_MAX_LEVELS) : 16, 1u << U(1, 3), 19, 512.0f, wild);
        cfg.early_stop_eps = coin(4) ? 1e-3f : 0.0f;
        cfg.mlp_exact_fp32 = coin(6); cfg.compact_live = coin(4);
        int32_t *t = &cfg.tuning.mlp_mode;
        for (size_t i = 0; i < sizeof(cfg.tuning) / sizeof(int32_t); ++i) t[i] = coin(3) ? (int32_t)U(0, 6) - (coin(6) ? 3 : 0) : 0;
        if (coin(4)) cfg.tuning.prop_sp_lanes = 8 << U(0, 2);
        io.rays_o = io.rays_d = (const float *)P();
        io.tile_w = coin(2) ? 0 : U(1, 900);
        io.N = coin(30) ? 0 : io.tile_w && !coin(20) ? io.tile_w * U(1, 900) : U(1, coin(3) ? 5000000 : 40000);
        io.skip_final = coin(8);
        if (!coin(30)) io.image = io.depth = io.weights_sum = (float *)P();
        for (uint32_t k = 0; k < SN_MAX_STAGES; ++k) {
            if (coin(5)) io.bins[k] = (float *)P();
            if (coin(8)) io.weights[k] = (float *)P();
            if (coin(8)) io.sigmas[k] = (float *)P();
            if (coin(8)) io.inds[k] = (int32_t *)P();
            if (coin(8)) { io.u_table[k] = (const float *)P(); if (coin(2)) io.u_ray_stride[k] = U(0, 700); }
        }
        if (coin(8)) { io.bins0_table = (const float *)P(); if (coin(2)) io.bins0_ray_stride = U(0, 700); }
        if (coin(8)) io.xyzs_last = (float *)P();
        if (coin(8)) io.geo_feat_last = (float *)P();
        if (coin(5)) io.f_image = (float *)P();
        if (!coin(10)) io.f_feat = (float *)P();
        if (coin(8)) io.head_stride = U(0, 200);
        if (coin(8)) io.out_stride = U(0, 8);
        sn_launch_info info;
        const int rc = sn_rm_render_route_info(&cfg, &io, &info);
        (void)sn_rm_render_workspace_bytes(&cfg, io.N, io.tile_w);
        rc == SN_OK ? ++ok : ++fail;
    }
    printf("plan_render_fuzz: %d configurations, %d planned, %d refused, no sanitizer report\n", iters, ok, fail);
    return ok > iters / 20 ? 0 : 1;
}
