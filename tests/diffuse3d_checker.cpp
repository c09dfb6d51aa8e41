/*
 * diffuse3d_checker.cpp — CPU restatement of the 3D step with the opt-in diffusion and buoyancy of the tracking channels
 * (include/fluidsim.h "3D channel diffusion and buoyancy").  TEST INFRASTRUCTURE ONLY.
 *
 * tests/st3d_checker.cpp (included unchanged, and through it oracle/sph_oracle3d.cpp) supplies Sim3, the sort network, the cell
 * walk, the surface-tension pass tension3 and the entry points st3_* and orc3_*.  step3 of the oracle is one function, so the
 * step is restated here once more, as st3d_checker.cpp restates it, with the pass between the surface-tension pass and the force
 * loop, statement for statement as the header writes it (f32, no contraction: build with -ffp-contract=off), and the `acc` line of
 * the integrate step with what the pass hands on: fb with a buoyancy channel, else st, else nothing.  With nothing set the step
 * is st3_step with enable == 0, operation for operation (tests/test_diffusion3d.py pins that byte for byte).
 * The carry (the sort's permutation applied to the channels) is the caller's: tests/diffuse3d_ref.py derives it from the records
 * before the step as tests/track3d_ref.py does, and hands in the channels in sorted-slot order.
 */
#include "st3d_checker.cpp"

namespace {

struct Diffuse3Settings {
    int channels;            /* C: rows of `attr`, each particle_count floats */
    float kappa[4];          /* conductivity per channel; 0: the channel is neither read nor written */
    int buoy;                /* buoyancy channel, -1: none */
    float beta, reference;
};

/* The pass on the state as the density loop left it: s.p sorted, densities and keys of this step, s.starts rebuilt.
 * attr: C x N in sorted-slot order; attr_out: C x N, rows of channels that do not diffuse are bit copies.  st: the surface-tension
 * forces of this step or NULL.  fb (may be NULL when buoy < 0): N.  R (may be NULL): per slot u_i sum_j w_j Cg d^2 in float64 from
 * the f32 weights; acc_out (may be NULL): C x N, the f32 sums (rows of channels that do not diffuse are +0). */
void diffuse3(const Sim3& s, const Diffuse3Settings& D, const float* attr, float* attr_out, const fs_vec3* st, fs_vec3* fb, double* R,
              float* acc_out) {
    const uint32_t N = s.st.particle_count;
    const float h = s.st.smoothing_radius;
    const float h2 = h * h;
    const float m = s.tk.mass;
    const float cg = 6.0f * s.poly6;
    const int C = D.channels;
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < C; ++c) g[c] = (2.0f * D.kappa[c]) * s.tk.delta;
    std::memcpy(attr_out, attr, sizeof(float) * (size_t)C * N);
#pragma omp parallel for schedule(dynamic, 1024)
    for (uint32_t i = 0; i < N; ++i) {
        const float* x = &s.p[i].predicted_position.x;
        uint32_t cc[3];
        cell_xyz(s, x, cc);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        double wsum = 0.0;
        for (int cz = -1; cz <= 1; ++cz)
            for (int cy = -1; cy <= 1; ++cy)
                for (int cx = -1; cx <= 1; ++cx) {
                    const uint32_t gx = cc[0] + cx, gy = cc[1] + cy, gz = cc[2] + cz;
                    if (gx >= s.gw || gy >= s.gh || gz >= s.gd) continue;
                    walk(s, s.p, cell_id(s, gx, gy, gz), [&](uint32_t j, const fs3_particle& nb) {
                        const float ox = nb.predicted_position.x - x[0], oy = nb.predicted_position.y - x[1],
                                    oz = nb.predicted_position.z - x[2];
                        const float r2 = ox * ox + oy * oy + oz * oz;
                        if (r2 > h2) return;
                        const float d = h2 - r2;
                        const float w = m / nb.density;
                        const float wk = w * ((cg * d) * d);
                        wsum += (double)wk;
                        for (int c = 0; c < C; ++c)
                            if (D.kappa[c] != 0.0f) acc[c] += wk * (attr[(size_t)c * N + j] - attr[(size_t)c * N + i]);
                    });
                }
        const float rho_i = s.p[i].density;
        const float ui = 1.0f / rho_i;
        for (int c = 0; c < C; ++c) {
            if (D.kappa[c] != 0.0f) attr_out[(size_t)c * N + i] = attr[(size_t)c * N + i] + (g[c] * acc[c]) * ui;
            if (acc_out) acc_out[(size_t)c * N + i] = acc[c];
        }
        if (R) R[i] = (double)ui * wsum;
        if (D.buoy >= 0) {
            const float a = attr[(size_t)D.buoy * N + i];
            const float sv = D.beta * (D.reference - a);
            const float rs = rho_i * sv;
            const float bx = rs * s.tk.gravity.x, by = rs * s.tk.gravity.y, bz = rs * s.tk.gravity.z;
            fb[i] = st ? fs_vec3{st[i].x + bx, st[i].y + by, st[i].z + bz} : fs_vec3{bx, by, bz};
        }
    }
}

/* step3 of the oracle as st3d_checker.cpp's step3_st restates it, with the pass behind the surface-tension pass and `+ hand` in the
 * acc line, hand = fb with a buoyancy channel, else st when surface tension is on, else nothing. */
void step3_df(Sim3& s, bool st_on, float sigma, float tau, const Diffuse3Settings& D, const float* attr, float* attr_out, fs_vec3* st_out,
              fs_vec3* fb_out, double* R, float* acc_out) {
    const uint32_t n = s.st.particle_count;
    const float dt = s.tk.delta, h = s.st.smoothing_radius;
    const float bs[3] = {s.st.size.x * 0.5f, s.st.size.y * 0.5f, s.st.size.z * 0.5f};
#pragma omp parallel for schedule(static)
    for (uint32_t i = 0; i < n; ++i) {
        fs3_particle& q = s.p[i];
        float* pr = &q.predicted_position.x;
        const float* po = &q.position.x;
        const float* ve = &q.velocity.x;
        for (int a = 0; a < 3; ++a) {
            pr[a] = po[a] + ve[a] * dt;
            if (std::fabs(pr[a]) > bs[a]) pr[a] = bs[a] * sgn(pr[a]);
        }
        uint32_t c[3];
        cell_xyz(s, pr, c);
        q.grid = cell_id(s, c[0], c[1], c[2]);
    }
    bitonic(s.p.data(), n, [](const fs3_particle& q) { return q.grid; });
    std::fill(s.starts.begin(), s.starts.end(), 0xFFFFFFFFu);
    for (uint32_t i = 0; i < n; ++i)
        if ((i == 0 || s.p[i].grid != s.p[i - 1].grid) && s.p[i].grid < s.starts.size()) s.starts[s.p[i].grid] = i;
    const float h2 = h * h;
#pragma omp parallel for schedule(dynamic, 1024)
    for (uint32_t i = 0; i < n; ++i) {
        const float* me = &s.p[i].predicted_position.x;
        uint32_t c[3];
        cell_xyz(s, me, c);
        float rho = 0.0f;
        for (int oz = -1; oz <= 1; ++oz)
            for (int oy = -1; oy <= 1; ++oy)
                for (int ox = -1; ox <= 1; ++ox) {
                    const uint32_t x = c[0] + ox, y = c[1] + oy, z = c[2] + oz;
                    if (x >= s.gw || y >= s.gh || z >= s.gd) continue;
                    walk(s, s.p, cell_id(s, x, y, z), [&](uint32_t, const fs3_particle& nb) {
                        const float dx = nb.predicted_position.x - me[0], dy = nb.predicted_position.y - me[1],
                                    dz = nb.predicted_position.z - me[2];
                        const float r2 = dx * dx + dy * dy + dz * dz;
                        float kern = 0.0f;
                        if (!(r2 > h2)) { const float d = h2 - r2; kern = s.poly6 * d * d * d; }
                        rho += s.tk.mass * kern * 1.0f;
                    });
                }
        rho = std::fmax(rho, EPS3);
        s.p[i].density = std::fmax(rho, 0.1f);
    }
    // ---- the surface-tension pass (st3d_checker.cpp), then the pass of this file
    std::vector<fs_vec3> stf, fbf;
    if (st_on) {
        stf.resize(n);
        tension3(s, sigma, tau, nullptr, nullptr, stf.data());
    }
    const bool any = D.buoy >= 0 || D.kappa[0] != 0.0f || D.kappa[1] != 0.0f || D.kappa[2] != 0.0f || D.kappa[3] != 0.0f || R || acc_out;
    if (D.buoy >= 0) fbf.resize(n);
    if (any) diffuse3(s, D, attr, attr_out, st_on ? stf.data() : nullptr, D.buoy >= 0 ? fbf.data() : nullptr, R, acc_out);
    else if (D.channels) std::memcpy(attr_out, attr, sizeof(float) * (size_t)D.channels * n);
    const fs_vec3* hand = D.buoy >= 0 ? fbf.data() : st_on ? stf.data() : nullptr;
    s.snap = s.p;
    const std::vector<fs3_particle>& src = s.snap;
#pragma omp parallel for schedule(dynamic, 1024)
    for (uint32_t i = 0; i < n; ++i) {
        fs3_particle q = src[i];
        const float* me = &q.predicted_position.x;
        const float pressure = s.tk.pressure_constant * (q.density - s.tk.rest_density);
        uint32_t seed = i * 12u + s.tick * 69u;
        float fp[3] = {0, 0, 0}, fv[3] = {0, 0, 0};
        uint32_t c[3];
        cell_xyz(s, me, c);
        for (int oz = -1; oz <= 1; ++oz)
            for (int oy = -1; oy <= 1; ++oy)
                for (int ox = -1; ox <= 1; ++ox) {
                    const uint32_t x = c[0] + ox, y = c[1] + oy, z = c[2] + oz;
                    if (x >= s.gw || y >= s.gh || z >= s.gd) continue;
                    walk(s, src, cell_id(s, x, y, z), [&](uint32_t k, const fs3_particle& nb) {
                        if (k == i) return;
                        const float o[3] = {nb.predicted_position.x - me[0], nb.predicted_position.y - me[1],
                                            nb.predicted_position.z - me[2]};
                        const float r2 = o[0] * o[0] + o[1] * o[1] + o[2] * o[2];
                        if (r2 > h2) return;
                        const float dst = std::sqrt(r2);
                        float dir[3];
                        if (dst == 0.0f) {
                            float r[3];
                            for (int a = 0; a < 3; ++a) {
                                seed ^= seed << 13; seed ^= seed >> 17; seed ^= seed << 5;
                                r[a] = (float)seed / 4294967296.0f;
                            }
                            const float len = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
                            for (int a = 0; a < 3; ++a) dir[a] = r[a] / len;
                        } else {
                            for (int a = 0; a < 3; ++a) dir[a] = o[a] / dst;
                        }
                        const float nrho = nb.density;
                        const float npress = s.tk.pressure_constant * (nrho - s.tk.rest_density);
                        const float kern = (dst <= h) ? (-(h - dst)) * s.spiky : 0.0f;
                        const float shared = (pressure + npress) * 0.5f;
                        float kv = 0.0f;
                        if (dst <= h)
                            kv = (dst == 0.0f) ? s.visc
                                               : s.visc * ((-(dst * dst * dst) / (2.0f * h * h * h)) + ((dst * dst) / (h * h)) +
                                                           (h / (2.0f * dst)) - 1.0f);
                        const float* nv = &nb.velocity.x;
                        const float* mv = &q.velocity.x;
                        for (int a = 0; a < 3; ++a) {
                            fp[a] += dir[a] * kern * shared / nrho;
                            fv[a] += (nv[a] - mv[a]) / nrho * kv;
                        }
                    });
                }
        float* v = &q.velocity.x;
        float* x = &q.position.x;
        const float g[3] = {s.tk.gravity.x, s.tk.gravity.y, s.tk.gravity.z};
        const float* hi = hand ? &hand[i].x : nullptr;
        for (int a = 0; a < 3; ++a) {
            float acc = fp[a] + fv[a] * s.tk.viscosity_coefficient;
            if (hand) acc = acc + hi[a];                                 // ---- added
            v[a] += (acc / q.density) * dt;
            v[a] += g[a] * dt;
        }
        if (!(v[0] == v[0] && v[1] == v[1] && v[2] == v[2])) v[0] = v[1] = v[2] = 0.0f;
        const float speed = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (speed > 500.0f) for (int a = 0; a < 3; ++a) v[a] = (v[a] / speed) * 500.0f;
        for (int a = 0; a < 3; ++a) x[a] += v[a] * dt;
        for (int a = 0; a < 3; ++a)
            if (std::fabs(x[a]) > bs[a]) { x[a] = bs[a] * sgn(x[a]); v[a] *= -1.0f * s.tk.damping_factor; }
        s.p[i] = q;
    }
    if (st_on && st_out) std::memcpy(st_out, stf.data(), n * sizeof(fs_vec3));
    if (D.buoy >= 0 && fb_out) std::memcpy(fb_out, fbf.data(), n * sizeof(fs_vec3));
}

}  // namespace

extern "C" {

/* One whole step, as orc3_step begins it.  st_on != 0: surface tension with (sigma, tau), its forces to st (may be NULL).  D, attr
 * (C x N, sorted-slot order), attr_out (C x N): the pass; fb (may be NULL), R, acc (each may be NULL): see diffuse3. */
void df3_step(void* hh, const fs3_tick_settings* t, int st_on, float sigma, float tau, const Diffuse3Settings* D, const float* attr,
              float* attr_out, fs_vec3* st, fs_vec3* fb, double* R, float* acc) {
    Sim3& s = *(Sim3*)hh;
    s.tick += 1;
    s.tk = *t;
    const float h = s.st.smoothing_radius;
    s.poly6 = 315.0f / (64.0f * PI3 * std::pow(h, 9.0f));
    s.spiky = 15.0f / (PI3 * std::pow(h, 5.0f));
    s.visc = 15.0f / (2.0f * PI3 * (h * h * h));
    step3_df(s, st_on != 0, sigma, tau, *D, attr, attr_out, st, fb, R, acc);
}

/* The tick counter (the seed of the coincident-pair PRNG): a checker re-seeded from a download goes on where the engine is. */
void df3_set_tick(void* hh, uint32_t tick) { ((Sim3*)hh)->tick = tick; }
uint32_t df3_tick(void* hh) { return ((Sim3*)hh)->tick; }

}  // extern "C"
