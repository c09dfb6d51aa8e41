/*
 * st_checker.cpp — CPU restatement of the opt-in surface-tension step.  TEST INFRASTRUCTURE ONLY.
 *
 * The oracle (oracle/sph_oracle.cpp, included unchanged) supplies the reference step: lattice, predict, spatial lookup,
 * both sorts, cell starts, density, the cell walk, pressure_force and viscosity_force; its orc_* entry points are
 * exported from this library as well.  Added here: the surface-tension pass, statement for statement as written in
 * DESIGN.md §11 (f32, no contraction: build with -ffp-contract=off), and move_particle with the ST term
 * ax = (fp.x + fv.x) + st.x.  With st == NULL the move is the oracle's, operation for operation.
 */
#include "../oracle/sph_oracle.cpp"

namespace {

// For every sorted slot i: n = sum_j m/rho_j grad W(q_i - q_j), L = sum_j m/rho_j lap W, over the cells and in the
// order of density() (3x3 sweep, walk_cell's start-index rules, i itself included).  Reads s.p after density().
void surface_tension(const OrcSim& s, fs_vec2* st, float* nl_out) {
    const fs_uniform& u = s.u;
    const float h2 = u.sqr_radius;
    const float cg = u.poly6_kernel_derivative;      // 24/(pi h^8)
    const float cl = 2.0f * cg;                      // 48/(pi h^8), exact
    const float sigma = u.surface_tension_coefficient, tau = u.surface_tension_treshold;
#pragma omp parallel for schedule(dynamic, 1024)
    for (uint32_t pi = 0; pi < u.particle_count; ++pi) {
        const fs_vec2 x = s.p[pi].predicted_position;
        uint32_t cxu, cyu;
        xy_of_point(u, x, &cxu, &cyu);
        const int32_t cx = (int32_t)cxu, cy = (int32_t)cyu;
        float nx = 0.0f, ny = 0.0f, L = 0.0f;
        for (int oy = -1; oy <= 1; ++oy)
            for (int ox = -1; ox <= 1; ++ox) {
                const uint32_t id = grid_pos_to_id(u, (uint32_t)(cx + ox), (uint32_t)(cy + oy));
                walk_cell(s, s.p, id, [&](uint32_t, const fs_particle& nb) {
                    const float ox_ = nb.predicted_position.x - x.x;
                    const float oy_ = nb.predicted_position.y - x.y;
                    const float r2 = ox_ * ox_ + oy_ * oy_;
                    if (r2 > h2) return;
                    const float d = h2 - r2;
                    const float w = u.particle_mass / nb.density;
                    const float k = (cg * d) * d;
                    nx += w * (k * ox_);
                    ny += w * (k * oy_);
                    const float lk = (cl * d) * ((3.0f * r2) - h2);
                    L += w * lk;
                });
            }
        const float nl = std::sqrt(nx * nx + ny * ny);
        fs_vec2 f{0.0f, 0.0f};
        if (nl > tau && nl > 0.0f) {
            const float sc = (-sigma * L) / nl;
            f = fs_vec2{sc * nx, sc * ny};
        }
        st[pi] = f;
        if (nl_out) { nl_out[3 * pi] = nx; nl_out[3 * pi + 1] = ny; nl_out[3 * pi + 2] = L; }
    }
}

// move_particles (sph_oracle.cpp, compute.wgsl:79-157) with the surface-tension force added to the force sum.
void move_particles_st(OrcSim& s, const fs_vec2* st) {
    const fs_uniform& u = s.u;
    s.snap = s.p;
    const std::vector<fs_particle>& src = s.snap;
#pragma omp parallel for schedule(dynamic, 1024)
    for (uint32_t id = 0; id < u.particle_count; ++id) {
        fs_particle q = src[id];
        const fs_vec2 fp = pressure_force(s, src, id);
        const fs_vec2 fv = viscosity_force(s, src, id);
        float ax = fp.x + fv.x, ay = fp.y + fv.y;
        if (st) { ax = ax + st[id].x; ay = ay + st[id].y; }
        q.velocity.x += (ax / q.density) * u.delta;
        q.velocity.y += (ay / q.density) * u.delta;
        q.velocity.x += u.gravity.x * u.delta;
        q.velocity.y += u.gravity.y * u.delta;
        if (u.mouse_state != 0) {
            const float dx = u.mouse_pos.x - q.predicted_position.x;
            const float dy = u.mouse_pos.y - q.predicted_position.y;
            const float dist = std::sqrt(dx * dx + dy * dy);
            if (dist <= u.mouse_force_radius) {
                const float dirx = dx / dist / dist, diry = dy / dist / dist;
                const float ratio = dist / u.mouse_force_radius;
                q.velocity.x += dirx * u.mouse_force_power * (float)u.mouse_state * ratio;
                q.velocity.y += diry * u.mouse_force_power * (float)u.mouse_state * ratio;
            }
        }
        if (!(q.velocity.x == q.velocity.x && q.velocity.y == q.velocity.y)) {
            q.velocity.x = 0.0f; q.velocity.y = 0.0f;
        }
        const float max_speed = 500.0f;
        const float speed = std::sqrt(q.velocity.x * q.velocity.x + q.velocity.y * q.velocity.y);
        if (speed > max_speed) {
            q.velocity.x = (q.velocity.x / speed) * max_speed;
            q.velocity.y = (q.velocity.y / speed) * max_speed;
        }
        q.position.x += q.velocity.x * u.delta;
        q.position.y += q.velocity.y * u.delta;

        const uint32_t tex_w = f32_to_u32_sat(u.texture_size.x);
        const float uvx = (q.predicted_position.x / u.bounds.x * 1.0f) + 0.5f;
        const float uvy = (q.predicted_position.y / u.bounds.y * 1.0f) + 0.5f;
        const uint32_t px = f32_to_u32_sat(uvx * u.texture_size.x);
        const uint32_t py = f32_to_u32_sat(uvy * u.texture_size.y);
        const uint32_t tix = py * tex_w + px;
        fs_vec2 force{0.0f, 0.0f};
        if (tix < s.texture.size()) force = s.texture[tix];
        const float p2wx = (u.bounds.x * 2.0f) / u.texture_size.x;
        const float p2wy = (u.bounds.y * 2.0f) / u.texture_size.y;
        const float fwx = force.x * p2wx, fwy = force.y * p2wy;
        if (force.x != 0.0f || force.y != 0.0f) {
            const float len = std::sqrt(force.x * force.x + force.y * force.y);
            const float nx = force.x / len, ny = force.y / len;
            q.position.x += fwx; q.position.y += fwy;
            const float vn = q.velocity.x * nx + q.velocity.y * ny;
            q.velocity.x -= (1.0f - u.damping_factor) * vn * nx;
            q.velocity.y -= (1.0f - u.damping_factor) * vn * ny;
        }
        const float bsx = u.bounds.x * 0.5f, bsy = u.bounds.y * 0.5f;
        if (std::fabs(q.position.x) > bsx) {
            q.position.x = bsx * sign_f32(q.position.x);
            q.velocity.x *= -1.0f * u.damping_factor;
        }
        if (std::fabs(q.position.y) > bsy) {
            q.position.y = bsy * sign_f32(q.position.y);
            q.velocity.y *= -1.0f * u.damping_factor;
        }
        s.p[id] = q;
    }
}

}  // namespace

extern "C" {

/* The ST pass on the oracle's current state (after orc_density): st[N]; nl (may be NULL): {n.x, n.y, L} per particle. */
void stc_surface_tension(orc_sim* h, fs_vec2* st, float* nl) { surface_tension(*(OrcSim*)h, st, nl); }

/* The move pass with the ST term (st == NULL: without it). */
void stc_move(orc_sim* h, const fs_vec2* st) { move_particles_st(*(OrcSim*)h, st); }

/* One whole step; st != NULL: surface tension on (its forces are written there), else the plain step. */
void stc_step(orc_sim* h, const fs_tick_settings* t, int stable_sort, fs_vec2* st) {
    orc_begin_tick(h, t);
    orc_predict(h);
    orc_spatial_lookup(h);
    if (stable_sort) orc_sort_stable(h); else orc_sort(h);
    orc_cell_starts(h);
    orc_density(h, 1);
    if (st) surface_tension(*(OrcSim*)h, st, nullptr);
    move_particles_st(*(OrcSim*)h, st);
}

}  // extern "C"
