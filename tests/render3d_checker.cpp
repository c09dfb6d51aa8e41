/*
 * render3d_checker.cpp — CPU restatement of 3D surface rendering (include/fluidsim.h).  TEST INFRASTRUCTURE ONLY.
 *
 * On top of the sampling checker (tests/sample3d_checker.cpp, which includes oracle/sph_oracle3d.cpp; both included unchanged):
 * its sample3_one is `sample(x)` of the statement and the `density` field of that record is `density(x)`.  Added here: the ray of
 * a pixel, the march, the bisection and the record, sequentially, one pixel after another, EVERY t_k evaluated — nothing is
 * skipped, so whatever the kernel skips has to be provably below iso.  f32, no contraction: build with -ffp-contract=off.
 */
#include "sample3d_checker.cpp"

namespace {

struct Ray3 { float o[3], d[3]; };

Ray3 pixel_ray(const fs3_camera& c, uint32_t i, uint32_t j) {
    const float u = ((float)i + 0.5f) / (float)c.width - 0.5f;
    const float v = ((float)j + 0.5f) / (float)c.height - 0.5f;
    const float eye[3] = {c.eye.x, c.eye.y, c.eye.z}, fw[3] = {c.forward.x, c.forward.y, c.forward.z};
    const float ri[3] = {c.right.x, c.right.y, c.right.z}, up[3] = {c.up.x, c.up.y, c.up.z};
    Ray3 r;
    float D[3];
    for (int a = 0; a < 3; ++a) {
        if (c.orthographic) { r.o[a] = (eye[a] + u * ri[a]) + v * up[a]; D[a] = fw[a]; }
        else { r.o[a] = eye[a]; D[a] = (fw[a] + u * ri[a]) + v * up[a]; }
    }
    const float len = std::sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
    for (int a = 0; a < 3; ++a) r.d[a] = D[a] / len;
    return r;
}

fs_vec3 at(const Ray3& r, float t) { return fs_vec3{r.o[0] + t * r.d[0], r.o[1] + t * r.d[1], r.o[2] + t * r.d[2]}; }

float density_at(const Sim3& s, const Ray3& r, float t) {
    fs3_sample S;
    sample3_one(s, at(r, t), &S);
    return S.density;
}

void render_one(const Sim3& s, const fs3_camera& c, const fs3_surface_params& p, uint32_t i, uint32_t j, fs3_surface_hit* out) {
    const Ray3 r = pixel_ray(c, i, j);
    uint32_t K = p.max_steps;
    for (uint32_t k = 0; k < p.max_steps; ++k)
        if (density_at(s, r, p.t_near + (float)k * p.ds) >= p.iso) { K = k; break; }
    fs3_surface_hit h;
    std::memset(&h, 0, sizeof h);                    // t, density, normal, velocity: +0
    h.steps = K;
    if (K == p.max_steps) { *out = h; return; }
    float t = p.t_near + (float)K * p.ds;
    h.hit = 2;
    if (K > 0) {
        float lo = p.t_near + (float)(K - 1) * p.ds, hi = t;
        for (uint32_t b = 0; b < p.refine; ++b) {
            const float mid = 0.5f * (lo + hi);
            if (density_at(s, r, mid) >= p.iso) hi = mid; else lo = mid;
        }
        t = hi;
        h.hit = 1;
    }
    fs3_sample S;
    sample3_one(s, at(r, t), &S);
    h.t = t;
    h.density = S.density;
    const float gl = std::sqrt((S.gradient.x * S.gradient.x + S.gradient.y * S.gradient.y) + S.gradient.z * S.gradient.z);
    if (gl > 0.0f) h.normal = fs_vec3{(-S.gradient.x) / gl, (-S.gradient.y) / gl, (-S.gradient.z) / gl};
    if (S.weight > 0.0f) h.velocity = fs_vec3{S.velocity.x / S.weight, S.velocity.y / S.weight, S.velocity.z / S.weight};
    *out = h;
}

}  // namespace

extern "C" {

/* The G-buffer of a camera on the state loaded by smp3_load, pixel (i, j) at j * width + i. */
void rnd3_render(void* hh, const fs3_camera* cam, const fs3_surface_params* sp, fs3_surface_hit* out) {
    const Sim3& s = *(const Sim3*)hh;
    const size_t w = cam->width, n = w * cam->height;
#pragma omp parallel for schedule(dynamic, 16)
    for (size_t q = 0; q < n; ++q) render_one(s, *cam, *sp, (uint32_t)(q % w), (uint32_t)(q / w), &out[q]);
}

/* The ray of pixel (i, j): o[3] then d[3]. */
void rnd3_ray(const fs3_camera* cam, uint32_t i, uint32_t j, float* o_d) {
    const Ray3 r = pixel_ray(*cam, i, j);
    for (int a = 0; a < 3; ++a) { o_d[a] = r.o[a]; o_d[3 + a] = r.d[a]; }
}

}  // extern "C"
