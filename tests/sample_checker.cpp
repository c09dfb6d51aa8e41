/*
 * sample_checker.cpp — CPU restatement of field sampling (include/fluidsim.h).  TEST INFRASTRUCTURE ONLY.
 *
 * The oracle (oracle/sph_oracle.cpp, included unchanged) supplies xy_of_point, grid_pos_to_id, walk_cell and poly6; its
 * orc_* entry points are exported from this library as well.  Added here: the sampler, operation for operation as the
 * header states it (f32, no contraction: build with -ffp-contract=off), the pixel centres of a view in orc_render's
 * expression, and a loader that puts a downloaded state (records, start indices, uniform) into an orc_sim.
 */
#include "../oracle/sph_oracle.cpp"

namespace {

void sample_one(const OrcSim& s, fs_vec2 x, int C, const float* attr, fs_sample* out, float* attr_out, size_t k_out, size_t n_out) {
    const fs_uniform& u = s.u;
    const size_t n = u.particle_count;
    const float h = u.smoothing_radius, h2 = h * h, m = u.particle_mass;
    uint32_t cxu, cyu;
    xy_of_point(u, x, &cxu, &cyu);
    const int32_t cx = (int32_t)cxu, cy = (int32_t)cyu;
    float density = 0.0f, weight = 0.0f, vx = 0.0f, vy = 0.0f, a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t neighbours = 0;
    for (int oy = -1; oy <= 1; ++oy)
        for (int ox = -1; ox <= 1; ++ox) {
            const uint32_t X = (uint32_t)(cx + ox), Y = (uint32_t)(cy + oy);
            if (X >= u.grid_w || Y >= u.grid_h) continue;                  // orc_render's rule
            walk_cell(s, s.p, grid_pos_to_id(u, X, Y), [&](uint32_t k, const fs_particle& nb) {
                const float dx = nb.predicted_position.x - x.x;
                const float dy = nb.predicted_position.y - x.y;
                const float r2 = dx * dx + dy * dy;
                if (r2 > h2) return;
                const float W = poly6(s, r2);                              // ((Cv * d) * d) * d
                density += m * W;
                const float t = (m / nb.density) * W;
                weight += t;
                vx += t * nb.velocity.x;
                vy += t * nb.velocity.y;
                for (int c = 0; c < C; ++c) a[c] += t * attr[(size_t)c * n + k];
                neighbours += 1;
            });
        }
    out->density = density; out->weight = weight;
    out->velocity.x = vx; out->velocity.y = vy;
    out->neighbours = neighbours;
    out->cell = grid_pos_to_id(u, cxu, cyu);
    for (int c = 0; c < C; ++c) attr_out[(size_t)c * n_out + k_out] = a[c];
}

}  // namespace

extern "C" {

/* A downloaded state into an orc_sim created with the same settings: records, start indices (len entries) and the uniform of
 * the step that produced them; poly6_norm as orc_begin_tick evaluates it. */
int smp_load(orc_sim* h, const fs_particle* p, size_t n, const uint32_t* start, size_t len, const fs_uniform* u) {
    OrcSim& s = *(OrcSim*)h;
    if (n != s.p.size() || len != s.start_indices.size() || u->particle_count != n) return 1;
    std::copy(p, p + n, s.p.begin());
    std::copy(start, start + len, s.start_indices.begin());
    s.u = *u;
    s.poly6_norm = 4.0f / (PI_F * std::pow(s.u.smoothing_radius, 8.0f));
    return 0;
}

/* attr: C channels of particle_count floats, channel c at c * particle_count (NULL with C == 0);
 * attr_out: channel c of query k at c * n + k. */
void smp_sample(orc_sim* h, const fs_vec2* pts, size_t n, int C, const float* attr, fs_sample* out, float* attr_out) {
    const OrcSim& s = *(const OrcSim*)h;
#pragma omp parallel for schedule(dynamic, 256)
    for (size_t k = 0; k < n; ++k) sample_one(s, pts[k], C, attr, &out[k], attr_out, k, n);
}

/* The pixel centres of a view, orc_render's expression; row-major at j * width + i. */
void smp_grid_points(float wminx, float wminy, float wmaxx, float wmaxy, uint32_t width, uint32_t height, fs_vec2* pts) {
    for (uint32_t j = 0; j < height; ++j)
        for (uint32_t i = 0; i < width; ++i) {
            fs_vec2 pt;
            pt.x = wminx + (((float)i + 0.5f) / (float)width) * (wmaxx - wminx);
            pt.y = wminy + (((float)j + 0.5f) / (float)height) * (wmaxy - wminy);
            pts[(size_t)j * width + i] = pt;
        }
}

void smp_sample_grid(orc_sim* h, float wminx, float wminy, float wmaxx, float wmaxy, uint32_t width, uint32_t height, int C,
                     const float* attr, fs_sample* out, float* attr_out) {
    const OrcSim& s = *(const OrcSim*)h;
    const size_t n = (size_t)width * height;
#pragma omp parallel for schedule(dynamic, 256)
    for (size_t q = 0; q < n; ++q) {
        const uint32_t i = (uint32_t)(q % width), j = (uint32_t)(q / width);
        fs_vec2 pt;
        pt.x = wminx + (((float)i + 0.5f) / (float)width) * (wmaxx - wminx);
        pt.y = wminy + (((float)j + 0.5f) / (float)height) * (wmaxy - wminy);
        sample_one(s, pt, C, attr, &out[q], attr_out, q, n);
    }
}

}  // extern "C"
