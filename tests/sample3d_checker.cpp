/*
 * sample3d_checker.cpp — CPU restatement of 3D field sampling (include/fluidsim.h).  TEST INFRASTRUCTURE ONLY.
 *
 * The 3D oracle (oracle/sph_oracle3d.cpp, included unchanged) supplies Sim3, cell_xyz, cell_id, walk and the constants; its
 * orc3_* entry points are exported from this library as well.  Added here: the sampler, operation for operation as the header
 * states it (f32, no contraction: build with -ffp-contract=off), the voxel centres of a view, and a loader that puts a
 * downloaded state (records, mass) into a Sim3 and rebuilds the clean cell starts as step3 does.
 */
#include "../oracle/sph_oracle3d.cpp"

namespace {

void sample3_one(const Sim3& s, fs_vec3 x, fs3_sample* out) {
    const float h = s.st.smoothing_radius, h2 = h * h, m = s.tk.mass;
    const float C6 = s.poly6, Cg = 6.0f * C6;
    const float pt[3] = {x.x, x.y, x.z};
    uint32_t c[3];
    cell_xyz(s, pt, c);
    float density = 0.0f, weight = 0.0f, v[3] = {0.0f, 0.0f, 0.0f}, gr[3] = {0.0f, 0.0f, 0.0f};
    uint32_t neighbours = 0;
    for (int oz = -1; oz <= 1; ++oz)
        for (int oy = -1; oy <= 1; ++oy)
            for (int ox = -1; ox <= 1; ++ox) {
                const uint32_t X = c[0] + ox, Y = c[1] + oy, Z = c[2] + oz;
                if (X >= s.gw || Y >= s.gh || Z >= s.gd) continue;
                walk(s, s.p, cell_id(s, X, Y, Z), [&](uint32_t, const fs3_particle& nb) {
                    const float dx = nb.predicted_position.x - x.x, dy = nb.predicted_position.y - x.y,
                                dz = nb.predicted_position.z - x.z;
                    const float r2 = dx * dx + dy * dy + dz * dz;
                    if (r2 > h2) return;
                    const float e = h2 - r2;
                    const float W = ((C6 * e) * e) * e;
                    density += m * W;
                    const float g = m * ((Cg * e) * e);
                    gr[0] += g * dx; gr[1] += g * dy; gr[2] += g * dz;
                    const float t = (m / nb.density) * W;
                    weight += t;
                    v[0] += t * nb.velocity.x; v[1] += t * nb.velocity.y; v[2] += t * nb.velocity.z;
                    neighbours += 1;
                });
            }
    out->density = density; out->weight = weight;
    out->velocity = fs_vec3{v[0], v[1], v[2]};
    out->gradient = fs_vec3{gr[0], gr[1], gr[2]};
    out->neighbours = neighbours;
    out->cell = cell_id(s, c[0], c[1], c[2]);
}

fs_vec3 voxel_centre(const fs3_view& v, uint32_t i, uint32_t j, uint32_t k) {
    fs_vec3 pt;
    pt.x = v.world_min.x + (((float)i + 0.5f) / (float)v.width) * (v.world_max.x - v.world_min.x);
    pt.y = v.world_min.y + (((float)j + 0.5f) / (float)v.height) * (v.world_max.y - v.world_min.y);
    pt.z = v.world_min.z + (((float)k + 0.5f) / (float)v.depth) * (v.world_max.z - v.world_min.z);
    return pt;
}

}  // namespace

extern "C" {

/* A downloaded state into a Sim3 created with the same settings: the records of fs3_download_particles after a step and the
 * mass of that step's tick.  The cell starts are rebuilt from the records as step3 does; poly6 as orc3_step evaluates it.
 * 1: the count does not fit; 2: the records are not sorted by `grid`. */
int smp3_load(void* hh, const fs3_particle* p, size_t n, float mass) {
    Sim3& s = *(Sim3*)hh;
    if (n != s.p.size()) return 1;
    for (size_t i = 1; i < n; ++i)
        if (p[i].grid < p[i - 1].grid) return 2;
    std::copy(p, p + n, s.p.begin());
    std::fill(s.starts.begin(), s.starts.end(), 0xFFFFFFFFu);
    for (uint32_t i = 0; i < n; ++i)
        if ((i == 0 || s.p[i].grid != s.p[i - 1].grid) && s.p[i].grid < s.starts.size()) s.starts[s.p[i].grid] = i;
    s.tk.mass = mass;
    s.poly6 = 315.0f / (64.0f * PI3 * std::pow(s.st.smoothing_radius, 9.0f));
    return 0;
}

void smp3_sample(void* hh, const fs_vec3* pts, size_t n, fs3_sample* out) {
    const Sim3& s = *(const Sim3*)hh;
#pragma omp parallel for schedule(dynamic, 256)
    for (size_t k = 0; k < n; ++k) sample3_one(s, pts[k], &out[k]);
}

/* The voxel centres of a view, voxel (i, j, k) at (k * height + j) * width + i. */
void smp3_grid_points(const fs3_view* view, fs_vec3* pts) {
    for (uint32_t k = 0; k < view->depth; ++k)
        for (uint32_t j = 0; j < view->height; ++j)
            for (uint32_t i = 0; i < view->width; ++i) pts[((size_t)k * view->height + j) * view->width + i] = voxel_centre(*view, i, j, k);
}

void smp3_sample_grid(void* hh, const fs3_view* view, fs3_sample* out) {
    const Sim3& s = *(const Sim3*)hh;
    const size_t w = view->width, wh = w * view->height, n = wh * view->depth;
#pragma omp parallel for schedule(dynamic, 256)
    for (size_t q = 0; q < n; ++q)
        sample3_one(s, voxel_centre(*view, (uint32_t)(q % w), (uint32_t)((q % wh) / w), (uint32_t)(q / wh)), &out[q]);
}

}  // extern "C"
