/*
 * mesh3d_checker.cpp — CPU restatement of 3D surface extraction (include/fluidsim.h).  TEST INFRASTRUCTURE ONLY.
 *
 * On top of the sampling checker (tests/sample3d_checker.cpp, which includes oracle/sph_oracle3d.cpp; both included unchanged):
 * its sample3_one is `sample(x)` of the statement, the `density` field of that record is `density(x)`, and its voxel_centre is
 * the node.  Added here: surface nets, serially, one cell after another and one lattice edge after another in the statement's
 * order, EVERY node evaluated.  f32, no contraction: build with -ffp-contract=off.
 */
#include "sample3d_checker.cpp"

#include <vector>

namespace {

struct Lattice {
    const fs3_view& v;
    uint32_t W, H, D;
    std::vector<float> F;
    std::vector<uint8_t> in;
    size_t node(uint32_t i, uint32_t j, uint32_t k) const { return ((size_t)k * H + j) * W + i; }
};

Lattice lattice_of(const Sim3& s, const fs3_view& v, float iso) {
    Lattice L{v, v.width, v.height, v.depth, {}, {}};
    const size_t n = (size_t)L.W * L.H * L.D;
    L.F.resize(n);
    L.in.resize(n);
#pragma omp parallel for schedule(dynamic, 256)
    for (size_t q = 0; q < n; ++q) {
        fs3_sample S;
        sample3_one(s, voxel_centre(v, (uint32_t)(q % L.W), (uint32_t)((q / L.W) % L.H), (uint32_t)(q / ((size_t)L.W * L.H))), &S);
        L.F[q] = S.density;
        L.in[q] = S.density >= iso ? 1 : 0;
    }
    return L;
}

bool cell_active(const Lattice& L, uint32_t i, uint32_t j, uint32_t k) {
    int inside = 0;
    for (uint32_t c = 0; c < 2; ++c)
        for (uint32_t b = 0; b < 2; ++b)
            for (uint32_t a = 0; a < 2; ++a) inside += L.in[L.node(i + a, j + b, k + c)];
    return inside != 0 && inside != 8;
}

/* The local position of an active cell's vertex: the mean of its edge crossings, in the statement's order of edges. */
void cell_local(const Lattice& L, float iso, uint32_t i, uint32_t j, uint32_t k, float l[3]) {
    float s[3] = {0.0f, 0.0f, 0.0f};
    uint32_t c = 0;
    for (int axis = 0; axis < 3; ++axis) {
        const int o1 = axis == 0 ? 1 : 0, o2 = axis == 2 ? 1 : 2;   /* the other two axes, ascending: (y,z), (x,z), (x,y) */
        for (uint32_t e = 0; e < 4; ++e) {
            uint32_t lo[3], hi[3];
            lo[axis] = 0; lo[o1] = e & 1u; lo[o2] = e >> 1;
            hi[0] = lo[0]; hi[1] = lo[1]; hi[2] = lo[2]; hi[axis] = 1;
            const size_t a = L.node(i + lo[0], j + lo[1], k + lo[2]), b = L.node(i + hi[0], j + hi[1], k + hi[2]);
            if (L.in[a] == L.in[b]) continue;
            const float tt = (iso - L.F[a]) / (L.F[b] - L.F[a]);
            c += 1;
            s[axis] += tt;
            s[o1] += (float)lo[o1];
            s[o2] += (float)lo[o2];
        }
    }
    for (int a = 0; a < 3; ++a) l[a] = s[a] / (float)c;
}

fs3_mesh_vertex cell_vertex(const Sim3& s, const Lattice& L, uint32_t i, uint32_t j, uint32_t k, const float l[3]) {
    const fs_vec3 n0 = voxel_centre(L.v, i, j, k), n1 = voxel_centre(L.v, i + 1, j + 1, k + 1);
    fs3_mesh_vertex o;
    std::memset(&o, 0, sizeof o);                   /* normal, velocity: +0 */
    o.position.x = n0.x + l[0] * (n1.x - n0.x);
    o.position.y = n0.y + l[1] * (n1.y - n0.y);
    o.position.z = n0.z + l[2] * (n1.z - n0.z);
    fs3_sample S;
    sample3_one(s, o.position, &S);
    o.density = S.density;
    const float gl = std::sqrt((S.gradient.x * S.gradient.x + S.gradient.y * S.gradient.y) + S.gradient.z * S.gradient.z);
    if (gl > 0.0f) o.normal = fs_vec3{(-S.gradient.x) / gl, (-S.gradient.y) / gl, (-S.gradient.z) / gl};
    if (S.weight > 0.0f) o.velocity = fs_vec3{S.velocity.x / S.weight, S.velocity.y / S.weight, S.velocity.z / S.weight};
    return o;
}

}  // namespace

extern "C" {

/* fs3_extract_surface on the state loaded by smp3_load: same arguments, same capacity rule.  cells / local (may be null): for
 * the written vertices, the cell index (k*(H-1) + j)*(W-1) + i and the local position l[3] of each. */
void msh3_extract(void* hh, const fs3_view* view, float iso, fs3_mesh_vertex* verts, uint32_t vert_cap, uint32_t* tris,
                  uint32_t tri_cap, uint32_t counts[2], uint32_t* cells, float* local) {
    const Sim3& s = *(const Sim3*)hh;
    const Lattice L = lattice_of(s, *view, iso);
    const uint32_t W = L.W, H = L.H, D = L.D;
    std::vector<uint32_t> rank((size_t)(W - 1) * (H - 1) * (D - 1), 0xFFFFFFFFu);
    uint32_t V = 0;
    for (uint32_t k = 0; k + 1 < D; ++k)
        for (uint32_t j = 0; j + 1 < H; ++j)
            for (uint32_t i = 0; i + 1 < W; ++i) {
                if (!cell_active(L, i, j, k)) continue;
                const size_t cell = ((size_t)k * (H - 1) + j) * (W - 1) + i;
                rank[cell] = V;
                if (V < vert_cap) {
                    float l[3];
                    cell_local(L, iso, i, j, k, l);
                    verts[V] = cell_vertex(s, L, i, j, k, l);
                    if (cells) cells[V] = (uint32_t)cell;
                    if (local) { local[3 * (size_t)V] = l[0]; local[3 * (size_t)V + 1] = l[1]; local[3 * (size_t)V + 2] = l[2]; }
                }
                V += 1;
            }
    uint32_t T = 0;
    const uint32_t ext[3] = {W, H, D};
    for (uint32_t k = 0; k < D; ++k)
        for (uint32_t j = 0; j < H; ++j)
            for (uint32_t i = 0; i < W; ++i)
                for (int A = 0; A < 3; ++A) {
                    const uint32_t n[3] = {i, j, k};
                    const int u = (A + 1) % 3, v = (A + 2) % 3;
                    if (n[A] + 1 >= ext[A]) continue;                                    /* no such edge */
                    if (n[u] < 1 || n[u] + 1 >= ext[u] || n[v] < 1 || n[v] + 1 >= ext[v]) continue;   /* not interior */
                    uint32_t m[3] = {i, j, k};
                    m[A] += 1;
                    const uint8_t in_lo = L.in[L.node(i, j, k)];
                    if (in_lo == L.in[L.node(m[0], m[1], m[2])]) continue;
                    auto vertex_of = [&](uint32_t du, uint32_t dv) {                     /* the cell at (u - du, v - dv) */
                        uint32_t c[3] = {i, j, k};
                        c[u] -= du; c[v] -= dv;
                        return rank[((size_t)c[2] * (H - 1) + c[1]) * (W - 1) + c[0]];
                    };
                    const uint32_t a = vertex_of(1, 1), b = vertex_of(0, 1), c = vertex_of(0, 0), d = vertex_of(1, 0);
                    const uint32_t q[4] = {a, in_lo ? b : d, c, in_lo ? d : b};
                    if (T < tri_cap) { tris[3 * (size_t)T] = q[0]; tris[3 * (size_t)T + 1] = q[1]; tris[3 * (size_t)T + 2] = q[2]; }
                    if (T + 1 < tri_cap) { tris[3 * (size_t)T + 3] = q[0]; tris[3 * (size_t)T + 4] = q[2]; tris[3 * (size_t)T + 5] = q[3]; }
                    T += 2;
                }
    counts[0] = V; counts[1] = T;
}

}  // extern "C"
