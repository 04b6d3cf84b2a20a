// scenes.cpp — seeded procedural stand-ins for the reference's absent assets,
// plus load_meshs (src/main.rs:494-561).
//
// The reference's benchmark scenes (README.md:27-34) are not in the tree
// (.MISSING_LARGE_BLOBS, .gitignore:2); every stand-in matches the triangle
// count of the scene it is named after and uses the camera of
// assets/scenes/<name>.ron.  All geometry comes from a PCG32 stream, so the
// GPU box regenerates bit-identical scenes from (name, n_tris, seed).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "scenes.h"

namespace trx {
namespace {

struct Pcg32 {
    uint64_t state, inc;
    explicit Pcg32(uint64_t seed, uint64_t seq = 54u) {
        state = 0;
        inc = (seq << 1u) | 1u;
        next();
        state += seed;
        next();
    }
    uint32_t next() {
        uint64_t old = state;
        state = old * 6364136223846793005ULL + inc;
        uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
        uint32_t rot = (uint32_t)(old >> 59u);
        return (xorshifted >> rot) | (xorshifted << ((32 - rot) & 31));
    }
    float uni() { return (float)(next() >> 8) * (1.0f / 16777216.0f); } // [0,1)
    float range(float a, float b) { return a + (b - a) * uni(); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
    float gauss() { // Box-Muller
        float u1 = std::max(uni(), 1e-7f), u2 = uni();
        return std::sqrt(-2.0f * std::log(u1)) * std::cos(6.2831853f * u2);
    }
};

struct V3 {
    float x, y, z;
};
inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 normalize(V3 a) {
    float l = std::sqrt(dot(a, a));
    return l > 0 ? a * (1.0f / l) : V3{0, 1, 0};
}

struct Mesh {
    std::vector<float> v;
    std::vector<uint64_t> objects; // triangle count per object
    uint64_t open_start = 0;
    uint64_t tris() const { return v.size() / 9; }
    void tri(V3 a, V3 b, V3 c) {
        float t[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
        v.insert(v.end(), t, t + 9);
    }
    void quad(V3 a, V3 b, V3 c, V3 d) {
        tri(a, b, c);
        tri(a, c, d);
    }
    void end_object() {
        uint64_t n = tris() - open_start;
        if (n) objects.push_back(n);
        open_start = tris();
    }
    void box(V3 lo, V3 hi) {
        V3 p[8];
        for (int i = 0; i < 8; i++) p[i] = {(i & 1) ? hi.x : lo.x, (i & 2) ? hi.y : lo.y, (i & 4) ? hi.z : lo.z};
        quad(p[0], p[2], p[3], p[1]);
        quad(p[4], p[5], p[7], p[6]);
        quad(p[0], p[1], p[5], p[4]);
        quad(p[2], p[6], p[7], p[3]);
        quad(p[0], p[4], p[6], p[2]);
        quad(p[1], p[3], p[7], p[5]);
    }
    // oriented box: centre c, half-axes ax, ay, az
    void obox(V3 c, V3 ax, V3 ay, V3 az) {
        V3 p[8];
        for (int i = 0; i < 8; i++)
            p[i] = c + ax * ((i & 1) ? 1.f : -1.f) + ay * ((i & 2) ? 1.f : -1.f) + az * ((i & 4) ? 1.f : -1.f);
        quad(p[0], p[2], p[3], p[1]);
        quad(p[4], p[5], p[7], p[6]);
        quad(p[0], p[1], p[5], p[4]);
        quad(p[2], p[6], p[7], p[3]);
        quad(p[0], p[4], p[6], p[2]);
        quad(p[1], p[3], p[7], p[5]);
    }
    // tessellated parallelogram with optional displacement callback
    template <class F> void grid(V3 o, V3 u, V3 w, int nu, int nw, F disp) {
        auto at = [&](int i, int j) {
            V3 p = o + u * ((float)i / nu) + w * ((float)j / nw);
            return disp(p, i, j);
        };
        for (int j = 0; j < nw; j++)
            for (int i = 0; i < nu; i++) quad(at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1));
    }
    void grid(V3 o, V3 u, V3 w, int nu, int nw) {
        grid(o, u, w, nu, nw, [](V3 p, int, int) { return p; });
    }
    // cylinder along axis from a to b
    void cylinder(V3 a, V3 b, float r, int seg, bool caps = true) {
        V3 ax = normalize(b - a);
        V3 t = std::fabs(ax.y) < 0.9f ? V3{0, 1, 0} : V3{1, 0, 0};
        V3 u = normalize(cross(ax, t)), w = cross(ax, u);
        for (int i = 0; i < seg; i++) {
            float a0 = 6.2831853f * i / seg, a1 = 6.2831853f * (i + 1) / seg;
            V3 d0 = u * (std::cos(a0) * r) + w * (std::sin(a0) * r);
            V3 d1 = u * (std::cos(a1) * r) + w * (std::sin(a1) * r);
            quad(a + d0, a + d1, b + d1, b + d0);
            if (caps) {
                tri(a, a + d1, a + d0);
                tri(b, b + d0, b + d1);
            }
        }
    }
    // UV sphere (2*seg*(rings-1) triangles)
    void sphere(V3 c, float r, int seg, int rings, V3 scale = {1, 1, 1}) {
        auto at = [&](int i, int j) {
            float th = 3.14159265f * j / rings, ph = 6.2831853f * i / seg;
            return V3{c.x + r * scale.x * std::sin(th) * std::cos(ph), c.y + r * scale.y * std::cos(th),
                      c.z + r * scale.z * std::sin(th) * std::sin(ph)};
        };
        for (int j = 0; j < rings; j++)
            for (int i = 0; i < seg; i++) {
                if (j > 0) tri(at(i, j), at(i + 1, j), at(i + 1, j + 1));
                if (j < rings - 1) tri(at(i, j), at(i + 1, j + 1), at(i, j + 1));
            }
    }
};

float hash2(int x, int y, uint32_t seed) {
    uint32_t h = (uint32_t)x * 374761393u + (uint32_t)y * 668265263u + seed * 2246822519u;
    h = (h ^ (h >> 13)) * 1274126177u;
    h ^= h >> 16;
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}
float vnoise(float x, float y, uint32_t seed) {
    int xi = (int)std::floor(x), yi = (int)std::floor(y);
    float fx = x - xi, fy = y - yi;
    float sx = fx * fx * (3 - 2 * fx), sy = fy * fy * (3 - 2 * fy);
    float a = hash2(xi, yi, seed), b = hash2(xi + 1, yi, seed), c = hash2(xi, yi + 1, seed),
          d = hash2(xi + 1, yi + 1, seed);
    return a + (b - a) * sx + (c - a) * sy + (a - b - c + d) * sx * sy;
}
float fbm(float x, float y, uint32_t seed, int oct) {
    float s = 0, a = 0.5f;
    for (int i = 0; i < oct; i++) {
        s += a * vnoise(x, y, seed + i);
        x *= 2.03f;
        y *= 2.03f;
        a *= 0.5f;
    }
    return s;
}

// ---- reusable props -----------------------------------------------------------
void leaf_cluster(Mesh &m, Pcg32 &rng, V3 c, V3 radii, uint64_t n_leaves, float leaf) {
    for (uint64_t i = 0; i < n_leaves; i++) {
        V3 d;
        do {
            d = {rng.range(-1, 1), rng.range(-1, 1), rng.range(-1, 1)};
        } while (dot(d, d) > 1.0f);
        V3 p = {c.x + d.x * radii.x, c.y + d.y * radii.y, c.z + d.z * radii.z};
        V3 a = normalize(V3{rng.range(-1, 1), rng.range(-1, 1), rng.range(-1, 1)});
        V3 b = normalize(cross(a, V3{rng.range(-1, 1), rng.range(-1, 1), rng.range(-1, 1)}));
        float s = leaf * std::exp(0.5f * rng.gauss());
        m.tri(p, p + a * s, p + b * s + a * (0.5f * s));
    }
}

void tree(Mesh &m, Pcg32 &rng, V3 base, float h, uint64_t n_leaves, float canopy = 1.0f, float leaf = 0.09f) {
    m.cylinder(base, base + V3{0, h * 0.55f, 0}, 0.12f * h / 5.0f + 0.05f, 12);
    int branches = 5;
    for (int b = 0; b < branches; b++) {
        float a = 6.28f * b / branches + rng.range(-0.3f, 0.3f);
        V3 s = base + V3{0, h * rng.range(0.35f, 0.55f), 0};
        V3 e = s + V3{std::cos(a) * h * 0.3f, h * rng.range(0.15f, 0.35f), std::sin(a) * h * 0.3f};
        m.cylinder(s, e, 0.04f, 8, false);
    }
    leaf_cluster(m, rng, base + V3{0, h * 0.75f, 0}, {h * 0.38f * canopy, h * 0.3f, h * 0.38f * canopy}, n_leaves, leaf);
}

void chair(Mesh &m, V3 c, float rot) {
    V3 ax = {std::cos(rot), 0, std::sin(rot)}, az = {-std::sin(rot), 0, std::cos(rot)}, ay = {0, 1, 0};
    auto P = [&](float x, float y, float z) { return c + ax * x + ay * y + az * z; };
    for (int i = 0; i < 4; i++) {
        float x = (i & 1) ? 0.2f : -0.2f, z = (i & 2) ? 0.2f : -0.2f;
        m.cylinder(P(x, 0, z), P(x, 0.45f, z), 0.015f, 6);
    }
    m.obox(P(0, 0.46f, 0), ax * 0.23f, ay * 0.012f, az * 0.23f);
    m.cylinder(P(-0.2f, 0.45f, -0.2f), P(-0.2f, 0.9f, -0.22f), 0.013f, 6);
    m.cylinder(P(0.2f, 0.45f, -0.2f), P(0.2f, 0.9f, -0.22f), 0.013f, 6);
    for (int k = 0; k < 4; k++) m.obox(P(0, 0.58f + 0.09f * k, -0.21f), ax * 0.2f, ay * 0.025f, az * 0.006f);
}

void table_set(Mesh &m, Pcg32 &rng, V3 c) {
    m.cylinder(c, c + V3{0, 0.72f, 0}, 0.03f, 10);
    m.cylinder(c + V3{0, 0.72f, 0}, c + V3{0, 0.75f, 0}, 0.4f, 24);
    m.cylinder(c, c + V3{0, 0.03f, 0}, 0.22f, 16);
    int chairs = 2 + (int)rng.below(3);
    for (int i = 0; i < chairs; i++) {
        float a = 6.28f * i / chairs + rng.range(-0.4f, 0.4f);
        chair(m, c + V3{std::cos(a) * 0.65f, 0, std::sin(a) * 0.65f}, a + 1.57f + rng.range(-0.3f, 0.3f));
    }
    // plates / glasses
    for (int i = 0; i < chairs; i++) {
        float a = 6.28f * i / chairs;
        V3 p = c + V3{std::cos(a) * 0.25f, 0.75f, std::sin(a) * 0.25f};
        m.cylinder(p, p + V3{0, 0.01f, 0}, 0.09f, 12);
        m.cylinder(p + V3{0.08f, 0, 0.08f}, p + V3{0.08f, 0.1f, 0.08f}, 0.025f, 8);
    }
}

void lamp(Mesh &m, V3 base) {
    m.cylinder(base, base + V3{0, 3.5f, 0}, 0.05f, 12);
    m.cylinder(base, base + V3{0, 0.4f, 0}, 0.1f, 12);
    m.sphere(base + V3{0, 3.7f, 0}, 0.2f, 16, 12);
}

// one building: facade grid of recessed windows, balconies, cornice, roof props
void building(Mesh &m, Pcg32 &rng, float x0, float x1, float zf, float zdir, float h, int detail) {
    float zb = zf + zdir * 10.0f;
    // shell
    m.box({x0, 0, std::min(zf, zb)}, {x1, h, std::max(zf, zb)});
    float floor_h = 3.2f;
    int floors = std::max(1, (int)(h / floor_h));
    float win_w = 1.2f, gap = 0.9f;
    int cols = std::max(1, (int)((x1 - x0 - gap) / (win_w + gap)));
    float zo = zf - zdir * 0.02f; // slightly in front of the facade
    for (int f = 0; f < floors; f++) {
        float y0 = f * floor_h + (f == 0 ? 0.3f : 0.9f), y1 = f * floor_h + 2.6f;
        for (int c = 0; c < cols; c++) {
            float wx0 = x0 + gap + c * (win_w + gap), wx1 = wx0 + win_w;
            // frame: four thin boxes + recessed pane + mullions
            float d = 0.12f * zdir;
            m.box({wx0 - 0.08f, y0 - 0.08f, std::min(zo, zo - d)}, {wx0, y1 + 0.08f, std::max(zo, zo - d)});
            m.box({wx1, y0 - 0.08f, std::min(zo, zo - d)}, {wx1 + 0.08f, y1 + 0.08f, std::max(zo, zo - d)});
            m.box({wx0, y1, std::min(zo, zo - d)}, {wx1, y1 + 0.08f, std::max(zo, zo - d)});
            m.box({wx0, y0 - 0.08f, std::min(zo, zo - d)}, {wx1, y0, std::max(zo, zo - d)});
            m.quad({wx0, y0, zo - d * 0.2f}, {wx1, y0, zo - d * 0.2f}, {wx1, y1, zo - d * 0.2f}, {wx0, y1, zo - d * 0.2f});
            for (int k = 1; k < detail; k++) {
                float mx = wx0 + (wx1 - wx0) * k / detail;
                m.box({mx - 0.015f, y0, std::min(zo, zo - d * 0.6f)}, {mx + 0.015f, y1, std::max(zo, zo - d * 0.6f)});
            }
            // shutters
            if (rng.uni() < 0.5f) {
                for (int s = 0; s < 2; s++) {
                    float sx = s ? wx1 + 0.1f : wx0 - 0.1f - 0.5f;
                    for (int l = 0; l < 4 * detail; l++) {
                        float ly = y0 + (y1 - y0) * l / (4 * detail);
                        m.box({sx, ly, std::min(zo, zo - d * 0.3f)}, {sx + 0.5f, ly + 0.04f, std::max(zo, zo - d * 0.3f)});
                    }
                }
            }
            // balcony with railing
            if (f > 0 && rng.uni() < 0.45f) {
                float bz0 = zo, bz1 = zo - zdir * 0.8f;
                m.box({wx0 - 0.3f, y0 - 0.9f, std::min(bz0, bz1)}, {wx1 + 0.3f, y0 - 0.8f, std::max(bz0, bz1)});
                int bars = 6 * detail;
                for (int b = 0; b <= bars; b++) {
                    float bx = wx0 - 0.3f + (win_w + 0.6f) * b / bars;
                    m.cylinder({bx, y0 - 0.8f, bz1}, {bx, y0 + 0.1f, bz1}, 0.012f, 6, false);
                }
                m.cylinder({wx0 - 0.3f, y0 + 0.1f, bz1}, {wx1 + 0.3f, y0 + 0.1f, bz1}, 0.02f, 8);
                // flower pots
                if (rng.uni() < 0.6f) {
                    V3 pc = {0.5f * (wx0 + wx1), y0 - 0.8f, 0.5f * (bz0 + bz1)};
                    m.cylinder(pc, pc + V3{0, 0.25f, 0}, 0.12f, 10);
                    leaf_cluster(m, rng, pc + V3{0, 0.45f, 0}, {0.25f, 0.2f, 0.25f}, 60 * (uint64_t)detail, 0.05f);
                }
            }
        }
        // string course per floor
        m.box({x0, f * floor_h + 3.0f, std::min(zo, zo - zdir * 0.1f)}, {x1, f * floor_h + 3.15f, std::max(zo, zo - zdir * 0.1f)});
    }
    // awning over ground floor
    if (rng.uni() < 0.7f) {
        float ay = 2.9f;
        V3 o = {x0 + 0.5f, ay, zo};
        m.grid(o, V3{x1 - x0 - 1.0f, 0, 0}, V3{0, -0.6f, -zdir * 1.6f}, 12 * detail, 6 * detail,
               [&](V3 p, int i, int) { return p + V3{0, 0.04f * std::sin(i * 1.3f), 0}; });
    }
    // roof clutter: chimneys
    int chim = 1 + (int)rng.below(3);
    for (int i = 0; i < chim; i++) {
        float cx = rng.range(x0 + 1, x1 - 1), cz = zf + zdir * rng.range(2, 8);
        m.box({cx - 0.3f, h, cz - 0.3f}, {cx + 0.3f, h + 1.2f, cz + 0.3f});
        m.cylinder({cx, h + 1.2f, cz}, {cx, h + 1.7f, cz}, 0.12f, 10);
    }
}

// fills the mesh up to exactly `target` triangles with single-leaf triangles
void pad_with_leaves(Mesh &m, Pcg32 &rng, uint64_t target, const std::vector<V3> &centres, V3 radii) {
    while (m.tris() < target) {
        V3 c = centres.empty() ? V3{0, 2, 0} : centres[rng.below((uint32_t)centres.size())];
        uint64_t chunk = std::min<uint64_t>(target - m.tris(), 256);
        leaf_cluster(m, rng, c, radii, chunk, 0.08f);
    }
}
void truncate(Mesh &m, uint64_t target) {
    if (m.tris() <= target) return;
    m.v.resize(target * 9);
    // drop / trim objects that were already closed beyond the cut
    uint64_t sum = 0;
    size_t keep = 0;
    for (; keep < m.objects.size(); keep++) {
        if (sum + m.objects[keep] > target) break;
        sum += m.objects[keep];
    }
    m.objects.resize(keep);
    m.open_start = sum;
}

// ---- scenes ---------------------------------------------------------------------
// "street": bistro-class stand-in.  Street along +x, camera in the street.
// `dense` (scene "bistro_dense") is the same street with the foliage where the camera looks: the canopies
// overhang the street and meet above it, as the big tree of the real Bistro exterior does in the reference's
// view (assets/scenes/bistro.ron), so most primary rays cross a leaf volume before they reach a facade.  Target
// (the PROFILE_RT legend of rt_gpu_software.hlsl:95,102 read on the reference's Bistro frames): about 30 node
// visits and 15 triangle tests per primary ray; tests/test_scenes.py pins both stand-ins.
void gen_bistro(Mesh &m, uint64_t target, uint64_t seed, bool per_object, bool dense = false) {
    Pcg32 rng(seed, 1);
    double scale = (double)target / 3872303.0;
    int detail = scale > 0.5 ? 3 : (scale > 0.1 ? 2 : 1);
    auto obj = [&]() {
        if (per_object) m.end_object();
    };
    // ground: cobbles with fbm height, finer near the street axis
    int gx = std::max(8, (int)(560 * std::sqrt(scale))), gz = std::max(4, (int)(280 * std::sqrt(scale)));
    m.grid({-45, 0, -28}, {110, 0, 0}, {0, 0, 56}, gx, gz,
           [&](V3 p, int, int) { return V3{p.x, 0.03f * fbm(p.x * 3, p.z * 3, 11, 3) - 0.015f, p.z}; });
    obj();
    // kerbs
    m.box({-45, 0, 4.6f}, {65, 0.15f, 4.9f});
    m.box({-45, 0, -4.9f}, {65, 0.15f, -4.6f});
    obj();
    // buildings on both sides
    std::vector<V3> tree_centres;
    for (int side = 0; side < 2; side++) {
        float zf = side ? -7.0f : 7.0f, zdir = side ? -1.0f : 1.0f;
        float x = -45;
        while (x < 62) {
            float w = rng.range(8, 15), h = rng.range(11, 20);
            building(m, rng, x, x + w, zf, zdir, h, detail);
            obj();
            x += w + (rng.uni() < 0.2f ? rng.range(1.5f, 3.0f) : 0.0f);
        }
    }
    // end wall far down the street so primary rays terminate on geometry
    building(m, rng, 62, 72, -12, 1, 18, detail);
    obj();
    building(m, rng, -58, -46, -12, 1, 16, detail);
    obj();
    // street furniture
    int n_tables = std::max(2, (int)(140 * scale));
    for (int i = 0; i < n_tables; i++) {
        float side = (i & 1) ? 1.0f : -1.0f;
        V3 c = {rng.range(-40, 58), 0.15f, side * rng.range(5.2f, 6.6f)};
        table_set(m, rng, c);
        obj();
    }
    int n_lamps = std::max(2, (int)(28 * std::sqrt(scale)));
    for (int i = 0; i < n_lamps; i++) {
        lamp(m, {-42.0f + 100.0f * i / n_lamps, 0.15f, (i & 1) ? 4.75f : -4.75f});
        obj();
    }
    // string lights across the street: catenaries of small bulbs
    int n_strings = std::max(1, (int)(40 * scale));
    for (int s = 0; s < n_strings; s++) {
        float x = rng.range(-40, 58), y = rng.range(5.5f, 7.5f);
        int bulbs = 24;
        for (int b = 0; b <= bulbs; b++) {
            float u = (float)b / bulbs;
            float z = -6.8f + 13.6f * u, sag = 0.9f * 4 * u * (1 - u);
            m.sphere({x + 0.3f * std::sin(u * 9), y - sag, z}, 0.045f, 8, 6);
            if (b < bulbs) {
                float u2 = (float)(b + 1) / bulbs;
                m.cylinder({x + 0.3f * std::sin(u * 9), y - sag, z},
                           {x + 0.3f * std::sin(u2 * 9), y - 0.9f * 4 * u2 * (1 - u2), -6.8f + 13.6f * u2}, 0.006f, 4, false);
            }
        }
        obj();
    }
    // trees / planters: roughly 45 % of the triangle budget is foliage, as in Bistro
    int n_trees = std::max(2, (int)(46 * std::sqrt(scale)));
    uint64_t used = m.tris();
    uint64_t foliage = target > used ? (uint64_t)((target - used) * 0.97) : 0;
    for (int i = 0; i < n_trees; i++) {
        float side = (i & 1) ? 1.0f : -1.0f;
        V3 base = {-41.0f + 100.0f * i / n_trees + rng.range(-1, 1), 0.15f, side * rng.range(5.0f, 6.2f)};
        float h = rng.range(4.5f, 7.5f);
        if (dense) {
            // trunks at the kerb, crowns 2.2 x as wide: neighbouring crowns interpenetrate and close over the street
            base.z = side * rng.range(3.6f, 4.8f);
            tree(m, rng, base, h, foliage / n_trees, 2.2f, 0.032f);
        } else {
            tree(m, rng, base, h, foliage / n_trees);
        }
        tree_centres.push_back(base + V3{0, h * 0.75f, 0});
        obj();
    }
    pad_with_leaves(m, rng, target, tree_centres, dense ? V3{4.4f, 1.6f, 4.4f} : V3{2.0f, 1.6f, 2.0f});
    truncate(m, target);
    m.end_object();
}

// kitchen-class room (56,939 triangles): closed room, cabinets, table, props.
void gen_kitchen(Mesh &m, uint64_t target, uint64_t seed, bool per_object) {
    Pcg32 rng(seed, 2);
    double scale = (double)target / 56939.0;
    auto obj = [&]() {
        if (per_object) m.end_object();
    };
    // room -5..4 x, 0..3 y, -3.5..3 z; tessellated floor (tiles)
    int t = std::max(2, (int)(40 * std::sqrt(scale)));
    m.grid({-5, 0, -3.5f}, {9, 0, 0}, {0, 0, 6.5f}, t, t);
    m.grid({-5, 3, -3.5f}, {0, 0, 6.5f}, {9, 0, 0}, 4, 4);
    m.grid({-5, 0, -3.5f}, {0, 3, 0}, {9, 0, 0}, 4, 4);
    m.grid({-5, 0, 3}, {9, 0, 0}, {0, 3, 0}, 4, 4);
    m.grid({-5, 0, -3.5f}, {0, 0, 6.5f}, {0, 3, 0}, 4, 4);
    m.grid({4, 0, -3.5f}, {0, 3, 0}, {0, 0, 6.5f}, 4, 4);
    obj();
    // cabinets along the far wall (x = -5) and back wall (z = -3.5)
    for (int i = 0; i < 10; i++) {
        float z0 = -3.3f + i * 0.62f;
        m.box({-4.95f, 0.1f, z0}, {-4.35f, 0.9f, z0 + 0.6f});
        m.box({-4.33f, 0.45f, z0 + 0.25f}, {-4.30f, 0.5f, z0 + 0.35f}); // handle
        m.box({-4.95f, 1.5f, z0}, {-4.6f, 2.3f, z0 + 0.6f});
        m.cylinder({-4.58f, 1.8f, z0 + 0.3f}, {-4.55f, 1.8f, z0 + 0.3f}, 0.02f, 8);
    }
    m.box({-4.97f, 0.9f, -3.32f}, {-4.3f, 0.95f, 2.9f}); // counter top
    obj();
    for (int i = 0; i < 8; i++) {
        float x0 = -4.2f + i * 0.82f;
        m.box({x0, 0.1f, -3.45f}, {x0 + 0.8f, 0.9f, -2.9f});
        m.cylinder({x0 + 0.4f, 0.6f, -2.88f}, {x0 + 0.4f, 0.6f, -2.85f}, 0.02f, 8);
    }
    m.box({-4.25f, 0.9f, -3.47f}, {2.4f, 0.95f, -2.85f});
    obj();
    // table + chairs in the middle
    m.box({-2.2f, 0.72f, -0.6f}, {0.2f, 0.78f, 0.8f});
    for (int i = 0; i < 4; i++)
        m.cylinder({(i & 1) ? 0.1f : -2.1f, 0, (i & 2) ? 0.7f : -0.5f}, {(i & 1) ? 0.1f : -2.1f, 0.72f, (i & 2) ? 0.7f : -0.5f}, 0.03f, 10);
    for (int i = 0; i < 6; i++) chair(m, {-1.9f + 0.85f * (i % 3), 0, (i < 3) ? -1.0f : 1.2f}, (i < 3) ? 0.0f : 3.14159f);
    obj();
    // props on counters and table: bowls, bottles, fruit
    int props = std::max(4, (int)(70 * scale));
    for (int i = 0; i < props; i++) {
        V3 p;
        int where = (int)rng.below(3);
        if (where == 0) p = {rng.range(-4.9f, -4.4f), 0.95f, rng.range(-3.2f, 2.8f)};
        else if (where == 1) p = {rng.range(-4.1f, 2.3f), 0.95f, rng.range(-3.4f, -2.95f)};
        else p = {rng.range(-2.1f, 0.1f), 0.78f, rng.range(-0.5f, 0.7f)};
        int kind = (int)rng.below(3);
        if (kind == 0) m.sphere(p + V3{0, 0.06f, 0}, 0.06f, 14, 10);
        else if (kind == 1) m.cylinder(p, p + V3{0, rng.range(0.15f, 0.3f), 0}, 0.035f, 14);
        else m.sphere(p + V3{0, 0.05f, 0}, 0.12f, 16, 8, {1, 0.4f, 1});
    }
    obj();
    // hanging lamp + window frames
    m.cylinder({-1, 3, 0.1f}, {-1, 2.2f, 0.1f}, 0.01f, 6);
    m.sphere({-1, 2.1f, 0.1f}, 0.18f, 20, 12);
    for (int i = 0; i < 3; i++) {
        float x0 = -3.5f + i * 2.3f;
        m.box({x0, 1.0f, 2.93f}, {x0 + 1.4f, 1.06f, 3.0f});
        m.box({x0, 2.2f, 2.93f}, {x0 + 1.4f, 2.26f, 3.0f});
        m.box({x0, 1.0f, 2.93f}, {x0 + 0.06f, 2.26f, 3.0f});
        m.box({x0 + 1.34f, 1.0f, 2.93f}, {x0 + 1.4f, 2.26f, 3.0f});
    }
    obj();
    std::vector<V3> centres = {{3.2f, 0.9f, 2.2f}, {3.3f, 0.9f, -2.6f}};
    m.cylinder({3.2f, 0, 2.2f}, {3.2f, 0.4f, 2.2f}, 0.2f, 16);
    m.cylinder({3.3f, 0, -2.6f}, {3.3f, 0.4f, -2.6f}, 0.2f, 16);
    pad_with_leaves(m, rng, target, centres, {0.45f, 0.5f, 0.45f});
    truncate(m, target);
    m.end_object();
}

// hairball-class: a tangle of thin four-sided tubes wandering through the WHOLE volume of a ball of radius 4.5
// (the real hairball.obj is 2.88 M triangles of such strands).  What makes the real asset the canonical worst case is
// kept: strands at every orientation, long thin triangles whose boxes are mostly empty, and gaps between strands,
// so a ray passes close to hundreds of strands on its way in.  Targets, checked by tests/test_scenes.py on the
// reference's camera (assets/scenes/hairball.ron: eye (0,0,7), fov 90): the ball's silhouette covers 31 % of a
// 16:9 frame and at least 90 % of those pixels must hit; node visits per primary ray at least 1.5 x the
// bistro-class scene's on the same builder.
void gen_hairball(Mesh &m, uint64_t target, uint64_t seed) {
    Pcg32 rng(seed, 3);
    const int seg = 180, sides = 4;
    const uint64_t per_strand = (uint64_t)seg * sides * 2;
    uint64_t strands = std::max<uint64_t>(1, target / per_strand);
    const float R = 4.5f;
    for (uint64_t s = 0; s < strands + 1 && m.tris() < target; s++) {
        // start anywhere in the ball (uniform in volume), head anywhere
        V3 p = normalize(V3{rng.gauss(), rng.gauss(), rng.gauss()}) * (R * std::cbrt(rng.range(0.0f, 1.0f)));
        V3 d = normalize(V3{rng.gauss(), rng.gauss(), rng.gauss()});
        V3 side = normalize(cross(d, V3{rng.gauss(), rng.gauss(), rng.gauss()}));
        const float step = rng.range(0.12f, 0.24f), wdt = rng.range(0.003f, 0.007f);
        const float curl = rng.range(0.08f, 0.35f);
        V3 ring[sides];
        bool have_ring = false;
        for (int k = 0; k < seg && m.tris() < target; k++) {
            V3 nd = normalize(d + V3{rng.gauss(), rng.gauss(), rng.gauss()} * curl);
            V3 q = p + nd * step;
            if (dot(q, q) > R * R) { // turn back inside: the silhouette stays a ball
                nd = normalize(nd - normalize(q) * 1.5f);
                q = p + nd * step;
            }
            side = normalize(cross(nd, cross(side, nd)));
            const V3 up = cross(nd, side);
            V3 next[sides];
            for (int a = 0; a < sides; a++) {
                const float ang = 6.2831853f * a / sides;
                const V3 off = side * (wdt * std::cos(ang)) + up * (wdt * std::sin(ang));
                if (!have_ring) ring[a] = p + off;
                next[a] = q + off;
            }
            have_ring = true;
            for (int a = 0; a < sides && m.tris() < target; a++) {
                const int b = (a + 1) % sides;
                m.tri(ring[a], ring[b], next[b]);
                if (m.tris() < target) m.tri(ring[a], next[b], next[a]);
            }
            for (int a = 0; a < sides; a++) ring[a] = next[a];
            p = q;
            d = nd;
        }
    }
    m.end_object();
}

// san-miguel-class courtyard: arcades, trees, tables; ~2000 objects
void gen_san_miguel(Mesh &m, uint64_t target, uint64_t seed) {
    Pcg32 rng(seed, 4);
    double scale = (double)target / 5075977.0;
    int detail = scale > 0.5 ? 3 : (scale > 0.1 ? 2 : 1);
    // courtyard floor (tiles) spanning x -25..30, z -30..20
    int g = std::max(8, (int)(420 * std::sqrt(scale)));
    m.grid({-25, 0, -30}, {55, 0, 0}, {0, 0, 50}, g, g,
           [&](V3 p, int, int) { return V3{p.x, 0.02f * fbm(p.x * 2, p.z * 2, 5, 3), p.z}; });
    m.end_object();
    // surrounding two-storey arcade buildings
    for (int side = 0; side < 4; side++) {
        for (int k = 0; k < 5; k++) {
            float a = -25.0f + 11.0f * k;
            if (side == 0) building(m, rng, a, a + 11, -30, -1, 9, detail);
            else if (side == 1) building(m, rng, a, a + 11, 20, 1, 9, detail);
            else {
                // x-facing sides: reuse z-facing generator on a swapped box by mirroring coordinates
                size_t before = m.v.size();
                float b = -30.0f + 10.0f * k;
                building(m, rng, b, b + 10, side == 2 ? -25.0f : 30.0f, side == 2 ? -1.0f : 1.0f, 9, detail);
                for (size_t i = before; i < m.v.size(); i += 3) std::swap(m.v[i], m.v[i + 2]);
            }
            m.end_object();
        }
    }
    // columns of the arcade
    for (int i = 0; i < 26; i++) {
        float x = -24.0f + 2.1f * i;
        m.cylinder({x, 0, -27}, {x, 3.5f, -27}, 0.18f, 20);
        m.end_object();
        m.cylinder({x, 0, 17}, {x, 3.5f, 17}, 0.18f, 20);
        m.end_object();
    }
    int n_tables = std::max(2, (int)(700 * scale));
    for (int i = 0; i < n_tables; i++) {
        table_set(m, rng, {rng.range(-20, 26), 0.02f, rng.range(-25, 15)});
        m.end_object();
    }
    int n_trees = std::max(2, (int)(900 * std::sqrt(scale)));
    uint64_t used = m.tris();
    uint64_t foliage = target > used ? (uint64_t)((target - used) * 0.97) : 0;
    std::vector<V3> centres;
    for (int i = 0; i < n_trees; i++) {
        V3 base = {rng.range(-22, 27), 0.02f, rng.range(-27, 17)};
        float h = rng.range(2.0f, 7.0f);
        tree(m, rng, base, h, foliage / n_trees);
        centres.push_back(base + V3{0, h * 0.75f, 0});
        m.end_object();
    }
    pad_with_leaves(m, rng, target, centres, {1.5f, 1.2f, 1.5f});
    truncate(m, target);
    m.end_object();
}

// Cornell-class box: 5 objects like assets/obj/cornell_box.obj (walls, sphere, two boxes, light)
void gen_cornell(Mesh &m, uint64_t target, uint64_t seed) {
    (void)seed;
    int t = 6;
    m.grid({-1, 0, -1}, {2, 0, 0}, {0, 0, 2}, t, t);   // floor
    m.grid({-1, 2, -1}, {0, 0, 2}, {2, 0, 0}, t, t);   // ceiling
    m.grid({-1, 0, -1}, {0, 2, 0}, {2, 0, 0}, t, t);   // back
    m.grid({-1, 0, -1}, {0, 0, 2}, {0, 2, 0}, t, t);   // left
    m.grid({1, 0, -1}, {0, 2, 0}, {0, 0, 2}, t, t);    // right
    m.end_object();
    int seg = 44, rings = 42; // 2*44*41 = 3608 triangles
    if (target && target < 3000) {
        seg = 12;
        rings = 8;
    }
    m.sphere({0.35f, 1.1f, 0.2f}, 0.3f, seg, rings);
    m.end_object();
    float c = std::cos(0.3f), s = std::sin(0.3f);
    m.obox({-0.35f, 0.6f, -0.3f}, V3{c, 0, s} * 0.3f, {0, 0.6f, 0}, V3{-s, 0, c} * 0.3f);
    m.end_object();
    m.obox({0.35f, 0.3f, 0.35f}, V3{c, 0, -s} * 0.3f, {0, 0.3f, 0}, V3{s, 0, c} * 0.3f);
    m.end_object();
    m.quad({-0.25f, 1.99f, -0.25f}, {0.25f, 1.99f, -0.25f}, {0.25f, 1.99f, 0.25f}, {-0.25f, 1.99f, 0.25f});
    m.end_object();
}

// demoscene stand-in: fBm height-field in [-1,1]^2 plus a few spheres
void gen_demoscene(Mesh &m, uint64_t target, uint64_t seed) {
    Pcg32 rng(seed, 6);
    uint64_t sph = 24 * (2 * 16 * 11);
    int res = (int)std::sqrt((double)(target > sph ? target - sph : target) / 2.0);
    res = std::max(res, 4);
    m.grid({-1, 0, -1}, {2, 0, 0}, {0, 0, 2}, res, res, [&](V3 p, int, int) {
        float h = fbm(p.x * 2.5f + 7, p.z * 2.5f + 3, (uint32_t)seed + 21, 7);
        return V3{p.x, 0.55f * h * h - 0.1f, p.z};
    });
    for (int i = 0; i < 24 && m.tris() + 2 * 16 * 11 <= target; i++) {
        V3 c = {rng.range(-0.8f, 0.8f), rng.range(0.15f, 0.4f), rng.range(-0.8f, 0.6f)};
        m.sphere(c, rng.range(0.02f, 0.06f), 16, 12);
    }
    std::vector<V3> centres = {{0, 0.3f, 0}};
    pad_with_leaves(m, rng, target, centres, {0.9f, 0.1f, 0.9f});
    truncate(m, target);
    m.end_object();
}

// random triangle soup in [-1,1]^3 (tests)
void gen_soup(Mesh &m, uint64_t target, uint64_t seed) {
    Pcg32 rng(seed, 7);
    for (uint64_t i = 0; i < target; i++) {
        V3 c = {rng.range(-1, 1), rng.range(-1, 1), rng.range(-1, 1)};
        float s = 0.02f + 0.25f * rng.uni() * rng.uni();
        auto off = [&]() { return V3{rng.range(-s, s), rng.range(-s, s), rng.range(-s, s)}; };
        m.tri(c + off(), c + off(), c + off());
    }
    m.end_object();
}

} // namespace

bool gen_scene(const std::string &name, uint64_t n_tris, uint64_t seed, std::vector<float> &verts,
               std::vector<uint64_t> &objects) {
    Mesh m;
    if (name == "bistro") gen_bistro(m, n_tris ? n_tris : 3872303, seed, true);
    else if (name == "bistro_dense") gen_bistro(m, n_tris ? n_tris : 3872303, seed, true, true);
    else if (name == "kitchen") gen_kitchen(m, n_tris ? n_tris : 56939, seed, true);
    else if (name == "hairball") gen_hairball(m, n_tris ? n_tris : 2880000, seed);
    else if (name == "san_miguel") gen_san_miguel(m, n_tris ? n_tris : 5075977, seed);
    else if (name == "cornell") gen_cornell(m, n_tris, seed);
    else if (name == "demoscene") gen_demoscene(m, n_tris ? n_tris : 2u * 2048u * 2048u, seed);
    else if (name == "soup") gen_soup(m, n_tris ? n_tris : 1000, seed);
    else return false;
    verts.swap(m.v);
    objects.swap(m.objects);
    return true;
}

// cameras of assets/scenes/*.ron:4-6 (demoscene: src/main.rs:249-254)
bool scene_camera(const std::string &name, float eye[3], float look_at[3], float *fov) {
    struct Cam {
        const char *n;
        float e[3], l[3], f;
    };
    static const Cam cams[] = {
        {"bistro", {-10.5f, 1.7f, -1.0f}, {12.5f, 1.7f, -2.0f}, 100.0f},
        {"bistro_dense", {-10.5f, 1.7f, -1.0f}, {12.5f, 1.7f, -2.0f}, 100.0f},
        {"kitchen", {3.0f, 1.5f, 1.4f}, {-3.9438584f, 1.5f, -1.7303504f}, 90.0f},
        {"hairball", {0.0f, 0.0f, 7.0f}, {0.0f, 0.0f, 0.0f}, 90.0f},
        {"san_miguel", {22.0f, 1.5f, 13.0f}, {-13.761939f, 1.5f, -22.647648f}, 90.0f},
        {"cornell", {0.0f, 1.0f, 2.1f}, {0.0f, 1.0f, 0.0f}, 90.0f},
        {"demoscene", {0.0f, 0.0f, 1.35f}, {0.0f, 0.16f, 0.35f}, 17.0f},
        {"soup", {0.0f, 0.0f, 3.0f}, {0.0f, 0.0f, 0.0f}, 60.0f},
    };
    for (const Cam &c : cams)
        if (name == c.n) {
            std::memcpy(eye, c.e, 12);
            std::memcpy(look_at, c.l, 12);
            *fov = c.f;
            return true;
        }
    return false;
}

// ---- load_meshs (src/main.rs:494-561) ---------------------------------------------
namespace {
// the rest of a line after its keyword, without surrounding blanks and the line end
std::string line_rest(const char *p) {
    std::string s(p);
    const size_t a = s.find_first_not_of(" \t"), b = s.find_last_not_of(" \t\r\n");
    return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
}

// One mtl file into names / table (6 floats per material: Kd, a missing one 0.8 each; Ke, a missing one 0).  A file that cannot
// be opened adds nothing.  false (mm.error set): a negative or non-finite Kd or Ke, more than 65535 named materials.
bool load_mtl(const std::string &path, std::vector<std::string> &names, ModelMaterials &mm, std::vector<std::string> *maps = nullptr) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return true;
    char line[4096];
    bool ok = true, open = false;
    while (ok && std::fgets(line, sizeof(line), f)) {
        const char *p = line;
        while (*p == ' ' || *p == '\t') p++;
        if (std::strncmp(p, "newmtl", 6) == 0 && (p[6] == ' ' || p[6] == '\t')) {
            if (names.size() >= 65535) {
                mm.error = "more than 65535 named materials";
                ok = false;
                break;
            }
            names.push_back(line_rest(p + 6));
            const float fresh[6] = {0.8f, 0.8f, 0.8f, 0.0f, 0.0f, 0.0f};
            mm.table.insert(mm.table.end(), fresh, fresh + 6);
            if (maps) maps->push_back(std::string());
            open = true;
        } else if (maps && open && std::strncmp(p, "map_Kd", 6) == 0 && (p[6] == ' ' || p[6] == '\t')) {
            // the file name is the last blank-separated word: options (-s 1 1 1, -bm 0.5, -clamp on ...) come before it
            const std::string rest = line_rest(p + 6);
            const size_t cut = rest.find_last_of(" \t");
            maps->back() = cut == std::string::npos ? rest : rest.substr(cut + 1);
        } else if (open && (p[0] == 'K') && (p[1] == 'd' || p[1] == 'e') && (p[2] == ' ' || p[2] == '\t')) {
            float c[3] = {0, 0, 0};
            const int got = std::sscanf(p + 2, "%f %f %f", &c[0], &c[1], &c[2]);
            for (int k = 0; k < 3; k++)
                if (got != 3 || !std::isfinite(c[k]) || c[k] < 0.0f) {
                    mm.error = std::string("material '") + names.back() + "': " + (p[1] == 'd' ? "Kd" : "Ke") + " is negative, not finite or not three numbers";
                    ok = false;
                }
            if (ok) std::memcpy(&mm.table[mm.table.size() - 6 + (p[1] == 'd' ? 0 : 3)], c, sizeof(c));
        }
    }
    std::fclose(f);
    return ok;
}

// mm (optional): the materials of trx_load_model_materials - `mtllib` files are read from the OBJ's directory as they are
// named, `usemtl` names are looked up once the whole file is read (the first material of a name wins; an unknown name, and
// faces before any usemtl, get material 0, the default).  The mesh is the same with and without it.
// mn (optional): the vertex normals of trx_load_model_normals - `vn` records, and the third index of a face corner's
// v/vt/vn or v//vn (relative when negative, against the `vn` records read so far); a corner without one, or with one out of
// range, gets +0.  The mesh is the same with and without it.
// mt (optional): the texture coordinates of trx_load_model_texcoords - `vt` records (two numbers; a missing second one is +0), and
// the second index of a face corner's v/vt or v/vt/vn, relative when negative; a corner without a usable one gets +0, +0.
// maps (optional, with mm): the map_Kd name per material of mm's table.
bool load_obj(const std::string &path, std::vector<float> &verts, std::vector<uint64_t> &objects, ModelMaterials *mm = nullptr,
              ModelNormals *mn = nullptr, ModelTexcoords *mt = nullptr, std::vector<std::string> *maps = nullptr) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<std::string> names, uses; // the mtl files' materials in file order; the names given to usemtl
    std::vector<uint32_t> tri_use;        // per triangle: 0 = before any usemtl, else 1 + index into uses
    uint32_t use = 0;
    if (mm) {
        const float fresh[6] = {0.8f, 0.8f, 0.8f, 0.0f, 0.0f, 0.0f};
        mm->table.assign(fresh, fresh + 6);
    }
    std::vector<float> pos, nrm, tex;
    if (maps) maps->assign(1, std::string());
    uint64_t open_start = 0;
    bool any_object = false;
    auto close_object = [&]() {
        uint64_t n = verts.size() / 9 - open_start;
        if (any_object || n) objects.push_back(n);
        open_start = verts.size() / 9;
    };
    char line[4096];
    while (std::fgets(line, sizeof(line), f)) {
        if (line[0] == 'v' && (line[1] == ' ' || line[1] == '\t')) {
            float x = 0, y = 0, z = 0;
            std::sscanf(line + 2, "%f %f %f", &x, &y, &z);
            pos.push_back(x);
            pos.push_back(y);
            pos.push_back(z);
        } else if (mn && line[0] == 'v' && line[1] == 'n' && (line[2] == ' ' || line[2] == '\t')) {
            float x = 0, y = 0, z = 0;
            std::sscanf(line + 3, "%f %f %f", &x, &y, &z);
            if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) {
                mn->error = "vn record " + std::to_string(nrm.size() / 3 + 1) + " is not finite";
                std::fclose(f);
                return false;
            }
            nrm.push_back(x);
            nrm.push_back(y);
            nrm.push_back(z);
        } else if (mt && line[0] == 'v' && line[1] == 't' && (line[2] == ' ' || line[2] == '\t')) {
            float s = 0, u = 0;
            std::sscanf(line + 3, "%f %f", &s, &u);
            tex.push_back(s);
            tex.push_back(u);
        } else if (line[0] == 'o' && (line[1] == ' ' || line[1] == '\t')) {
            if (any_object || verts.size() / 9 > open_start) close_object();
            any_object = true;
        } else if (mm && std::strncmp(line, "mtllib", 6) == 0 && (line[6] == ' ' || line[6] == '\t')) {
            const size_t slash = path.find_last_of('/');
            const std::string dir = slash == std::string::npos ? std::string() : path.substr(0, slash + 1);
            if (!load_mtl(dir + line_rest(line + 6), names, *mm, maps)) {
                std::fclose(f);
                return false;
            }
        } else if (mm && std::strncmp(line, "usemtl", 6) == 0 && (line[6] == ' ' || line[6] == '\t')) {
            uses.push_back(line_rest(line + 6));
            use = (uint32_t)uses.size();
        } else if (line[0] == 'f' && (line[1] == ' ' || line[1] == '\t')) {
            long idx[4], nidx[4] = {-1, -1, -1, -1}, tidx[4] = {-1, -1, -1, -1}; // (nidx, tidx: the corner's `vn` and `vt`, -1 = none)
            int n = 0;
            char *p = line + 2;
            for (;;) { // n counts every vertex of the polygon; the first four are kept
                while (*p == ' ' || *p == '\t') p++;
                if (*p == 0 || *p == '\n' || *p == '\r') break;
                char *end;
                long v = std::strtol(p, &end, 10);
                if (end == p) break;
                if (v < 0) v = (long)(pos.size() / 3) + v + 1; // relative index
                if (n < 4) idx[n] = v - 1;
                n++;
                p = end;
                if (mt && n <= 4 && *p == '/') { // v/vt or v/vt/vn: the second index
                    char *tend;
                    long vt = std::strtol(p + 1, &tend, 10);
                    if (tend != p + 1) {
                        if (vt < 0) vt = (long)(tex.size() / 2) + vt + 1; // relative index
                        tidx[n - 1] = vt - 1;
                    }
                }
                if (mn && n <= 4 && *p == '/') { // v/vt/vn or v//vn: the third index
                    const char *q = p + 1;
                    while (*q && *q != '/' && *q != ' ' && *q != '\t' && *q != '\n' && *q != '\r') q++;
                    if (*q == '/') {
                        char *nend;
                        long vn = std::strtol(q + 1, &nend, 10);
                        if (nend != q + 1) {
                            if (vn < 0) vn = (long)(nrm.size() / 3) + vn + 1; // relative index
                            nidx[n - 1] = vn - 1;
                        }
                    }
                }
                while (*p && *p != ' ' && *p != '\t' && *p != '\n' && *p != '\r') p++; // skip /vt/vn
            }
            auto push = [&](int ka, int kb, int kc) {
                const long a = idx[ka], b = idx[kb], c = idx[kc];
                long np = (long)(pos.size() / 3);
                if (a < 0 || b < 0 || c < 0 || a >= np || b >= np || c >= np) return;
                for (long i : {a, b, c}) {
                    verts.push_back(pos[3 * i]);
                    verts.push_back(pos[3 * i + 1]);
                    verts.push_back(pos[3 * i + 2]);
                }
                if (mm) tri_use.push_back(use);
                if (mn)
                    for (int k : {ka, kb, kc}) {
                        const long i = nidx[k];
                        const bool have = i >= 0 && i < (long)(nrm.size() / 3);
                        mn->any = mn->any || have;
                        for (int j = 0; j < 3; j++) mn->normals.push_back(have ? nrm[3 * i + j] : 0.0f);
                    }
                if (mt)
                    for (int k : {ka, kb, kc}) {
                        const long i = tidx[k];
                        const bool have = i >= 0 && i < (long)(tex.size() / 2);
                        mt->any = mt->any || have;
                        for (int j = 0; j < 2; j++) mt->uvs.push_back(have ? tex[2 * i + j] : 0.0f);
                    }
            };
            // the reference reads vertices 0,1,2 and, for quads only, 0,2,3 (src/main.rs:536-553)
            if (n >= 3) push(0, 1, 2);
            if (n == 4) push(0, 2, 3);
        }
    }
    std::fclose(f);
    close_object();
    if (objects.empty()) objects.push_back(0);
    if (mm) {
        std::vector<uint16_t> of_use(uses.size() + 1, 0);
        for (size_t u = 0; u < uses.size(); u++)
            for (size_t m = 0; m < names.size(); m++)
                if (names[m] == uses[u]) {
                    of_use[u + 1] = (uint16_t)(m + 1);
                    break;
                }
        mm->tri.resize(tri_use.size());
        for (size_t i = 0; i < tri_use.size(); i++) mm->tri[i] = of_use[tri_use[i]];
    }
    return true;
}

// `[{"v0":[x,y,z], "v1":[...], "v2":[...]}, ...]` (src/main.rs:502-527)
bool load_json(const std::string &path, std::vector<float> &verts, std::vector<uint64_t> &objects) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string s;
    char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
    std::fclose(f);
    size_t pos = 0;
    for (;;) {
        float t[9];
        bool ok = true;
        for (int k = 0; k < 3 && ok; k++) {
            char key[8];
            std::snprintf(key, sizeof(key), "\"v%d\"", k);
            size_t p = s.find(key, pos);
            if (p == std::string::npos) {
                ok = false;
                break;
            }
            p = s.find('[', p);
            if (p == std::string::npos) {
                ok = false;
                break;
            }
            const char *c = s.c_str() + p + 1;
            char *end;
            for (int j = 0; j < 3; j++) {
                t[3 * k + j] = std::strtof(c, &end);
                c = end;
                while (*c == ',' || *c == ' ') c++;
            }
            pos = (size_t)(c - s.c_str());
        }
        if (!ok) break;
        verts.insert(verts.end(), t, t + 9);
    }
    objects.push_back(verts.size() / 9);
    return true;
}
} // namespace

bool load_model(const std::string &path, std::vector<float> &verts, std::vector<uint64_t> &objects) {
    if (path.find("json") != std::string::npos && path.rfind('.') != std::string::npos &&
        path.substr(path.rfind('.')).find("json") != std::string::npos)
        return load_json(path, verts, objects);
    return load_obj(path, verts, objects);
}

bool load_model_materials(const std::string &path, std::vector<float> &verts, std::vector<uint64_t> &objects, ModelMaterials &mm) {
    mm = ModelMaterials();
    if (path.find("json") != std::string::npos && path.rfind('.') != std::string::npos &&
        path.substr(path.rfind('.')).find("json") != std::string::npos) {
        if (!load_json(path, verts, objects)) return false;
        const float fresh[6] = {0.8f, 0.8f, 0.8f, 0.0f, 0.0f, 0.0f};
        mm.table.assign(fresh, fresh + 6);
        mm.tri.assign(verts.size() / 9, 0);
        return true;
    }
    return load_obj(path, verts, objects, &mm);
}

bool load_model_normals(const std::string &path, std::vector<float> &verts, std::vector<uint64_t> &objects, ModelNormals &mn) {
    mn = ModelNormals();
    if (path.find("json") != std::string::npos && path.rfind('.') != std::string::npos &&
        path.substr(path.rfind('.')).find("json") != std::string::npos) {
        if (!load_json(path, verts, objects)) return false;
        mn.normals.assign(verts.size(), 0.0f);
        return true;
    }
    return load_obj(path, verts, objects, nullptr, &mn);
}

bool load_model_texcoords(const std::string &path, std::vector<float> &verts, std::vector<uint64_t> &objects, ModelTexcoords &mt) {
    mt = ModelTexcoords();
    if (path.find("json") != std::string::npos && path.rfind('.') != std::string::npos &&
        path.substr(path.rfind('.')).find("json") != std::string::npos) {
        if (!load_json(path, verts, objects)) return false;
        mt.uvs.assign(verts.size() / 9 * 6, 0.0f);
        return true;
    }
    return load_obj(path, verts, objects, nullptr, nullptr, &mt);
}

bool load_model_material_maps(const std::string &path, std::vector<std::string> &maps, std::string &error) {
    std::vector<float> verts;
    std::vector<uint64_t> objects;
    maps.assign(1, std::string());
    if (path.find("json") != std::string::npos && path.rfind('.') != std::string::npos &&
        path.substr(path.rfind('.')).find("json") != std::string::npos)
        return load_json(path, verts, objects);
    ModelMaterials mm;
    const bool ok = load_obj(path, verts, objects, &mm, nullptr, nullptr, &maps);
    error = mm.error;
    return ok;
}

// Vertex normals from the mesh alone (include/trx.h, trx_compute_vertex_normals).  Every operation in binary64, rounded
// once, no contraction (this file's flags); dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
void compute_vertex_normals(const float *verts, uint64_t n_tris, double crease_cos, float *out) {
    struct V3 {
        double x, y, z;
    };
    auto dot = [](const V3 &a, const V3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; };
    // face vectors cross(v1 - v0, v2 - v0) and their unit vectors; len == 0 marks a face that contributes nowhere
    std::vector<V3> face(n_tris), unit(n_tris);
    std::vector<uint8_t> valid(n_tris);
    for (uint64_t t = 0; t < n_tris; t++) {
        const float *v = verts + 9 * t;
        const V3 e1{(double)v[3] - (double)v[0], (double)v[4] - (double)v[1], (double)v[5] - (double)v[2]};
        const V3 e2{(double)v[6] - (double)v[0], (double)v[7] - (double)v[1], (double)v[8] - (double)v[2]};
        const V3 f{e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
        const double len = std::sqrt(dot(f, f));
        valid[t] = std::isfinite(len) && len > 0.0;
        face[t] = f;
        unit[t] = valid[t] ? V3{f.x / len, f.y / len, f.z / len} : V3{0.0, 0.0, 0.0};
    }
    // welding: one id per distinct position (bitwise, -0.0 taken as +0.0) among the corners of the valid faces, through an
    // open-addressing table keyed by a hash of the position bits
    const uint64_t n_corners = n_tris * 3;
    uint64_t cap = 16;
    while (cap < n_corners * 2) cap *= 2;
    const uint32_t kEmpty = 0xffffffffu;
    std::vector<uint32_t> table(cap, kEmpty); // -> the first corner seen at the position
    std::vector<uint32_t> vid(n_corners, kEmpty), first_corner;
    auto key = [&](uint64_t corner, uint32_t k[3]) {
        for (int j = 0; j < 3; j++) {
            std::memcpy(&k[j], verts + 3 * corner + j, 4);
            if (k[j] == 0x80000000u) k[j] = 0u;
        }
    };
    for (uint64_t c = 0; c < n_corners; c++) {
        if (!valid[c / 3]) continue;
        uint32_t k[3], o[3];
        key(c, k);
        uint64_t h = ((uint64_t)k[0] * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)k[1] * 0xC2B2AE3D27D4EB4Full) ^ ((uint64_t)k[2] * 0x165667B19E3779F9ull);
        h ^= h >> 29;
        for (uint64_t slot = h & (cap - 1);; slot = (slot + 1) & (cap - 1)) {
            if (table[slot] == kEmpty) {
                table[slot] = (uint32_t)first_corner.size();
                vid[c] = (uint32_t)first_corner.size();
                first_corner.push_back((uint32_t)c);
                break;
            }
            key(first_corner[table[slot]], o);
            if (o[0] == k[0] && o[1] == k[1] && o[2] == k[2]) {
                vid[c] = table[slot];
                break;
            }
        }
    }
    // the triangles at every position, ascending (a valid face has three distinct positions: listed once)
    const uint64_t n_vid = first_corner.size();
    std::vector<uint64_t> start(n_vid + 1, 0);
    for (uint64_t c = 0; c < n_corners; c++)
        if (vid[c] != kEmpty) start[vid[c] + 1]++;
    for (uint64_t i = 0; i < n_vid; i++) start[i + 1] += start[i];
    std::vector<uint32_t> list(start[n_vid]);
    {
        std::vector<uint64_t> fill(start.begin(), start.end() - 1);
        for (uint64_t c = 0; c < n_corners; c++)
            if (vid[c] != kEmpty) list[fill[vid[c]]++] = (uint32_t)(c / 3);
    }
    for (uint64_t c = 0; c < n_corners; c++) {
        float *o = out + 3 * c;
        o[0] = o[1] = o[2] = 0.0f;
        const uint64_t t = c / 3;
        if (!valid[t]) continue;
        V3 sum{0.0, 0.0, 0.0};
        for (uint64_t i = start[vid[c]]; i < start[vid[c] + 1]; i++) {
            const uint32_t t2 = list[i];
            if (t2 != t && !(dot(unit[t2], unit[t]) >= crease_cos)) continue;
            sum.x += face[t2].x;
            sum.y += face[t2].y;
            sum.z += face[t2].z;
        }
        const double len = std::sqrt(dot(sum, sum));
        if (!(std::isfinite(len) && len > 0.0)) continue;
        o[0] = (float)(sum.x / len);
        o[1] = (float)(sum.y / len);
        o[2] = (float)(sum.z / len);
    }
}

// The subset of RON the reference's scene files use (assets/scenes/*.ron): model_path, camera(eye, look_at, fov,
// exposure), sun_direction; `//` comments.  "If we got a relative path to both the scene and the model, assume the path to
// the model is relative to the path to the scene" - three levels up (src/main.rs:271-284).
bool parse_scene_ron(const std::string &path, std::string &model_path, float eye[3], float look_at[3], float *fov_deg) {
    std::ifstream f(path);
    if (!f) return false;
    std::stringstream ss;
    std::string line;
    while (std::getline(f, line)) {
        const size_t c = line.find("//");
        if (c != std::string::npos) line.erase(c);
        ss << line << '\n';
    }
    const std::string s = ss.str();
    auto tuple3 = [&](const char *key, float out[3]) {
        size_t k = s.find(key);
        if (k == std::string::npos) return false;
        k = s.find('(', k);
        if (k == std::string::npos) return false;
        return std::sscanf(s.c_str() + k, "( %f , %f , %f", &out[0], &out[1], &out[2]) == 3;
    };
    size_t k = s.find("model_path");
    if (k == std::string::npos) return false;
    const size_t q0 = s.find('"', k), q1 = q0 == std::string::npos ? q0 : s.find('"', q0 + 1);
    if (q1 == std::string::npos) return false;
    model_path = s.substr(q0 + 1, q1 - q0 - 1);
    if (!tuple3("eye", eye) || !tuple3("look_at", look_at)) return false;
    k = s.find("fov");
    const size_t colon = k == std::string::npos ? k : s.find(':', k);
    if (colon == std::string::npos || std::sscanf(s.c_str() + colon + 1, " %f", fov_deg) != 1) return false;
    if (!path.empty() && path[0] != '/' && !model_path.empty() && model_path[0] != '/') {
        std::string base = path;
        for (int up = 0; up < 3; up++) {
            const size_t sl = base.find_last_of('/');
            base = sl == std::string::npos ? std::string() : base.substr(0, sl);
        }
        if (!base.empty()) model_path = base + "/" + model_path;
    }
    return true;
}


} // namespace trx
