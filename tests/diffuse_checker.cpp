/*
 * diffuse_checker.cpp — CPU restatement of the opt-in diffusion and buoyancy of the tracking channels.
 * TEST INFRASTRUCTURE ONLY.
 *
 * tests/st_checker.cpp (included unchanged, and through it oracle/sph_oracle.cpp) supplies the reference step, the
 * surface-tension pass and move_particles_st, whose `st` operand is what this pass hands on as fb.  Added here: the pass,
 * statement for statement as written in include/fluidsim.h (f32, no contraction: build with -ffp-contract=off), and the part
 * of a whole step behind the sort: cell starts -> density -> optional ST -> diffusion / buoyancy -> move_particles_st(fb).
 * The carry (the sort's permutation applied to the channels) is the caller's: tests/diffuse_ref.py derives it from the keys as
 * tests/track_ref.py does.
 */
#include "st_checker.cpp"

namespace {

struct DiffuseSettings {
    int channels;            /* C: rows of `attr`, each particle_count floats */
    float kappa[4];          /* conductivity per channel; 0: the channel is neither read nor written */
    int buoy;                /* buoyancy channel, -1: none */
    float beta, reference;
};

/* attr: C x N, the values the carry delivered, in sorted-slot order; attr_out: C x N, rows of channels that do not diffuse are
 * bit copies.  st: the surface-tension forces of this step or NULL.  fb (may be NULL when buoy < 0): N.  R (may be NULL): per
 * slot u_i sum_j w_j Cg d^2 in float64 from the f32 weights; acc (may be NULL): C x N, the f32 sums (rows of channels that do
 * not diffuse are +0).  Reads s.p after density(). */
void diffuse(const OrcSim& s, const DiffuseSettings& D, const float* attr, float* attr_out, const fs_vec2* st, fs_vec2* fb, double* R,
             float* acc_out) {
    const fs_uniform& u = s.u;
    const uint32_t N = u.particle_count;
    const float h2 = u.sqr_radius;
    const float cg = u.poly6_kernel_derivative;      /* 24/(pi h^8) */
    const int C = D.channels;
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < C; ++c) g[c] = (2.0f * D.kappa[c]) * u.delta;
    std::memcpy(attr_out, attr, sizeof(float) * (size_t)C * N);
#pragma omp parallel for schedule(dynamic, 1024)
    for (uint32_t pi = 0; pi < N; ++pi) {
        const fs_vec2 x = s.p[pi].predicted_position;
        uint32_t cxu, cyu;
        xy_of_point(u, x, &cxu, &cyu);
        const int32_t cx = (int32_t)cxu, cy = (int32_t)cyu;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        double wsum = 0.0;
        for (int oy = -1; oy <= 1; ++oy)
            for (int ox = -1; ox <= 1; ++ox) {
                const uint32_t id = grid_pos_to_id(u, (uint32_t)(cx + ox), (uint32_t)(cy + oy));
                walk_cell(s, s.p, id, [&](uint32_t j, const fs_particle& nb) {
                    const float ox_ = nb.predicted_position.x - x.x;
                    const float oy_ = nb.predicted_position.y - x.y;
                    const float r2 = ox_ * ox_ + oy_ * oy_;
                    if (r2 > h2) return;
                    const float d = h2 - r2;
                    const float w = u.particle_mass / nb.density;
                    const float wk = w * ((cg * d) * d);
                    wsum += (double)wk;
                    for (int c = 0; c < C; ++c)
                        if (D.kappa[c] != 0.0f) acc[c] += wk * (attr[(size_t)c * N + j] - attr[(size_t)c * N + pi]);
                });
            }
        const float rho_i = s.p[pi].density;
        const float ui = 1.0f / rho_i;
        for (int c = 0; c < C; ++c) {
            if (D.kappa[c] != 0.0f) attr_out[(size_t)c * N + pi] = attr[(size_t)c * N + pi] + (g[c] * acc[c]) * ui;
            if (acc_out) acc_out[(size_t)c * N + pi] = acc[c];
        }
        if (R) R[pi] = (double)ui * wsum;
        if (D.buoy >= 0) {
            const float a = attr[(size_t)D.buoy * N + pi];
            const float sv = D.beta * (D.reference - a);
            const float bx = (rho_i * sv) * u.gravity.x, by = (rho_i * sv) * u.gravity.y;
            fb[pi] = st ? fs_vec2{st[pi].x + bx, st[pi].y + by} : fs_vec2{bx, by};
        }
    }
}

}  // namespace

extern "C" {

/* The pass on the oracle's current state (after orc_density). */
void dfc_diffuse(orc_sim* h, const DiffuseSettings* D, const float* attr, float* attr_out, const fs_vec2* st, fs_vec2* fb, double* R,
                 float* acc) {
    diffuse(*(OrcSim*)h, *D, attr, attr_out, st, fb, R, acc);
}

/* The rest of a whole step behind the sort (the caller has run orc_begin_tick, orc_predict, orc_spatial_lookup and a sort, and
 * carried `attr` through the sort's permutation): cell starts, density, the ST pass when st != NULL (its forces are written
 * there), the diffusion / buoyancy pass, and the move with what the pass hands on: fb with a buoyancy channel, else st. */
void dfc_finish_step(orc_sim* h, const DiffuseSettings* D, const float* attr, float* attr_out, fs_vec2* st, fs_vec2* fb, double* R,
                     float* acc) {
    orc_cell_starts(h);
    orc_density(h, 1);
    if (st) surface_tension(*(OrcSim*)h, st, nullptr);
    diffuse(*(OrcSim*)h, *D, attr, attr_out, st, fb, R, acc);
    move_particles_st(*(OrcSim*)h, D->buoy >= 0 ? fb : st);
}

}  // extern "C"
