/*
 * st3d_checker.cpp — CPU restatement of the 3D step with the opt-in surface-tension pass (include/fluidsim.h "3D surface
 * tension").  TEST INFRASTRUCTURE ONLY.
 *
 * The 3D oracle (oracle/sph_oracle3d.cpp, included unchanged) supplies Sim3, the sort network, the cell walk and the cell
 * coordinates; its orc3_* entry points are exported from this library as well.  step3 of the oracle is one function, so the step
 * is restated here with two additions: the surface-tension pass between the density and the force loop, statement for statement
 * as the header writes it (f32, no contraction: build with -ffp-contract=off), and the `acc` line of the integrate step,
 * acc = (fp + fv * viscosity_coefficient) + st.  With enable == 0 the step is the oracle's, operation for operation
 * (tests/test_surface_tension3d.py pins that byte for byte).
 */
#include "../oracle/sph_oracle3d.cpp"

namespace {

// The pass on the state as the density loop left it: s.p sorted, densities and keys of this step, s.starts rebuilt.
// n_out (may be null): 3 floats per slot; L_out (may be null): one; st: one fs_vec3.
void tension3(const Sim3& s, float sigma, float tau, float* n_out, float* L_out, fs_vec3* st) {
    const uint32_t n = s.st.particle_count;
    const float h = s.st.smoothing_radius;
    const float h2 = h * h;
    const float m = s.tk.mass;
    const float cg = 6.0f * s.poly6;
    const float h2x3 = 3.0f * h2;
#pragma omp parallel for schedule(dynamic, 1024)
    for (uint32_t i = 0; i < n; ++i) {
        const float* x = &s.p[i].predicted_position.x;
        uint32_t c[3];
        cell_xyz(s, x, c);
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, L = 0.0f;
        for (int cz = -1; cz <= 1; ++cz)
            for (int cy = -1; cy <= 1; ++cy)
                for (int cx = -1; cx <= 1; ++cx) {
                    const uint32_t gx = c[0] + cx, gy = c[1] + cy, gz = c[2] + cz;
                    if (gx >= s.gw || gy >= s.gh || gz >= s.gd) continue;
                    walk(s, s.p, cell_id(s, gx, gy, gz), [&](uint32_t, const fs3_particle& nb) {
                        const float ox = nb.predicted_position.x - x[0], oy = nb.predicted_position.y - x[1],
                                    oz = nb.predicted_position.z - x[2];
                        const float r2 = ox * ox + oy * oy + oz * oz;
                        if (r2 > h2) return;
                        const float d = h2 - r2;
                        const float w = m / nb.density;
                        const float k = (cg * d) * d;
                        nx += w * (k * ox);
                        ny += w * (k * oy);
                        nz += w * (k * oz);
                        const float lk = (cg * d) * ((7.0f * r2) - h2x3);
                        L += w * lk;
                    });
                }
        const float nl = std::sqrt((nx * nx + ny * ny) + nz * nz);
        fs_vec3 f{0.0f, 0.0f, 0.0f};
        if (nl > tau && nl > 0.0f) {
            const float sc = (-sigma * L) / nl;
            f = fs_vec3{sc * nx, sc * ny, sc * nz};
        }
        st[i] = f;
        if (n_out) { n_out[3 * i] = nx; n_out[3 * i + 1] = ny; n_out[3 * i + 2] = nz; }
        if (L_out) L_out[i] = L;
    }
}

// step3 of the oracle, restated: the pass after the density loop, `+ st` in the acc line.  enable == false: neither.
void step3_st(Sim3& s, bool enable, float sigma, float tau, std::vector<fs_vec3>& stf, float* acc_out) {
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
    // ---- added: the surface-tension pass
    if (enable) {
        stf.resize(n);
        tension3(s, sigma, tau, nullptr, nullptr, stf.data());
    }
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
        const float* sti = enable ? &stf[i].x : nullptr;
        for (int a = 0; a < 3; ++a) {
            float acc = fp[a] + fv[a] * s.tk.viscosity_coefficient;
            if (enable) acc = acc + sti[a];                              // ---- added
            if (acc_out) acc_out[3 * (size_t)i + a] = acc;               // (a copy for the tests: nothing reads it back)
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
}

}  // namespace

extern "C" {

/* One whole step, as orc3_step begins it.  enable != 0: surface tension with (sigma, tau); st (may be NULL) receives the forces,
 * one fs_vec3 per sorted slot.  enable == 0: the oracle's step; sigma, tau and st are not looked at.  acc (may be NULL) receives
 * the step's `acc` values, 3 floats per sorted slot. */
void st3_step(void* hh, const fs3_tick_settings* t, int enable, float sigma, float tau, fs_vec3* st, float* acc) {
    Sim3& s = *(Sim3*)hh;
    s.tick += 1;
    s.tk = *t;
    const float h = s.st.smoothing_radius;
    s.poly6 = 315.0f / (64.0f * PI3 * std::pow(h, 9.0f));
    s.spiky = 15.0f / (PI3 * std::pow(h, 5.0f));
    s.visc = 15.0f / (2.0f * PI3 * (h * h * h));
    std::vector<fs_vec3> stf;
    step3_st(s, enable != 0, sigma, tau, stf, acc);
    if (enable && st) std::memcpy(st, stf.data(), stf.size() * sizeof(fs_vec3));
}

/* The pass alone on the records as they are — sorted by key, with the densities to weigh with (the state a step leaves: its
 * predicted positions, densities and keys belong together); the cell starts are rebuilt from the keys, the mass and the poly6
 * constant are those of the last step.  n: 3 floats per slot, L: one, st: one fs_vec3; each may be NULL except st. */
void st3_pass(void* hh, float sigma, float tau, float* n, float* L, fs_vec3* st) {
    Sim3& s = *(Sim3*)hh;
    const uint32_t cnt = s.st.particle_count;
    std::fill(s.starts.begin(), s.starts.end(), 0xFFFFFFFFu);
    for (uint32_t i = 0; i < cnt; ++i)
        if ((i == 0 || s.p[i].grid != s.p[i - 1].grid) && s.p[i].grid < s.starts.size()) s.starts[s.p[i].grid] = i;
    tension3(s, sigma, tau, n, L, st);
}

}  // extern "C"
