// gs4d_host.cpp — host-side (CPU) half of the path: the splat parameterisation and camera matrices the
// reference computes with GLM before anything reaches the GPU.  Part of libgs4d.so so that callers without
// GLM (the Python binding, the C++ scene driver) can build SSBO contents that are bit-identical to the
// reference's.  Pinned by tests/golden/* (generated from the reference's own code).
//
//   Splat4D::Splat4D (rot,scale,lifetime,fade,dir)   4DSplatRendering/Splat.h:132-159
//   Splat4D::Splat4D (rot0,rot1,scalar)              4DSplatRendering/Splat.h:91-130
//   Splat3D::Splat3D                                 4DSplatRendering/Splat.h:334-344
//   Camera::GetViewMatrix / GetProjMatrix            4DSplatRendering/Camera.cpp:50-58
//   orientation of teapot splats                     4DSplatRendering/Scenes.h:268
//   SplatData record layout                          4DSplatRendering/Scenes.h:22-37
// GLM 0.9.9.9 evaluation order is reproduced (float32, no contraction: build with -ffp-contract=off).
// The record builders, the transforms and the queries that a device call evaluates too are the kernels' own headers (../csrc/*.h), compiled here.
#include "../../include/gs4d.h"
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
#include "../csrc/build_record.h"
#include "../csrc/decompose_record.h"
#include "../csrc/transform_record.h"
#include "../csrc/pose_record.h"
#include "../csrc/sh_rotate_record.h"
#include "../csrc/sh_rotate_operands.h"
#include "../csrc/sh_time_record.h"
#include "../csrc/warp_record.h"
#include "../csrc/slice_record.h"
#include "../csrc/centre_query.h"
#include "../csrc/measure_record.h"
#include "../csrc/merge_record.h"
#include "../csrc/merge_rows_record.h"
#include "../csrc/lod_query.h"
#include "../csrc/neighbour_query.h"
#include "../csrc/component_union.h"
#include "../csrc/nearest_query.h"

namespace {

using gs4d_build::M3;        // column-major, element (col c, row r) = a[c * 3 + r]
using gs4d_build::Quat;
struct Vec3 { float x, y, z; };

inline Vec3 sub(Vec3 a, Vec3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline float dot(Vec3 a, Vec3 b) { const float p0 = a.x * b.x, p1 = a.y * b.y, p2 = a.z * b.z; return p0 + p1 + p2; }
inline Vec3 cross(Vec3 a, Vec3 b) { return { a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y }; }
inline Vec3 scale(Vec3 a, float s) { return { a.x * s, a.y * s, a.z * s }; }
inline Vec3 unit(Vec3 a) { return scale(a, 1.0f / std::sqrt(dot(a, a))); }

Quat quat_of(const M3& m) {   // glm::quat_cast
    auto at = [&m](int c, int r) { return m.a[c * 3 + r]; };
    const float tx = at(0, 0) - at(1, 1) - at(2, 2);
    const float ty = at(1, 1) - at(0, 0) - at(2, 2);
    const float tz = at(2, 2) - at(0, 0) - at(1, 1);
    const float tw = at(0, 0) + at(1, 1) + at(2, 2);
    int which = 0; float best = tw;
    if (tx > best) { best = tx; which = 1; }
    if (ty > best) { best = ty; which = 2; }
    if (tz > best) { best = tz; which = 3; }
    const float big = std::sqrt(best + 1.0f) * 0.5f;
    const float k = 0.25f / big;
    if (which == 0) return { big, (at(1, 2) - at(2, 1)) * k, (at(2, 0) - at(0, 2)) * k, (at(0, 1) - at(1, 0)) * k };
    if (which == 1) return { (at(1, 2) - at(2, 1)) * k, big, (at(0, 1) + at(1, 0)) * k, (at(2, 0) + at(0, 2)) * k };
    if (which == 2) return { (at(2, 0) - at(0, 2)) * k, (at(0, 1) + at(1, 0)) * k, big, (at(1, 2) + at(2, 1)) * k };
    return { (at(0, 1) - at(1, 0)) * k, (at(2, 0) + at(0, 2)) * k, (at(1, 2) + at(2, 1)) * k, big };
}

} // namespace

extern "C" {

void gs4d_host_look_at(const float eye[3], const float orientation[3], const float up[3], float view[16]) {
    const Vec3 e = { eye[0], eye[1], eye[2] };
    const Vec3 centre = { eye[0] + orientation[0], eye[1] + orientation[1], eye[2] + orientation[2] };
    const Vec3 f = unit(sub(centre, e));
    const Vec3 s = unit(cross(f, { up[0], up[1], up[2] }));
    const Vec3 u = cross(s, f);
    const float m[16] = { s.x, u.x, -f.x, 0.0f, s.y, u.y, -f.y, 0.0f, s.z, u.z, -f.z, 0.0f, -dot(s, e), -dot(u, e), dot(f, e), 1.0f };
    std::memcpy(view, m, sizeof m);
}

void gs4d_host_perspective(float fov_deg, int width, int height, float znear, float zfar, float proj[16]) {
    const float fovy = fov_deg * 0.01745329251994329576923690768489f;
    const float aspect = (float)width / (float)height;
    const float th = std::tan(fovy / 2.0f);
    float m[16] = { 0 };
    m[0] = 1.0f / (aspect * th);
    m[5] = 1.0f / th;
    m[10] = -(zfar + znear) / (zfar - znear);
    m[11] = -1.0f;
    m[14] = -(2.0f * zfar * znear) / (zfar - znear);
    std::memcpy(proj, m, sizeof m);
}

// Picking: the world point at view depth `depth` (= -z_view, what gs4d_read_aux's D/O is) on the ray through the centre of
// pixel (px, py) — window coordinates (px + 0.5, py + 0.5), row 0 at the bottom, as the images are.  In double: with z_view fixed, the two
// NDC equations are linear in (x_view, y_view) for any projection matrix; the view matrix is inverted by Gauss-Jordan elimination.
void gs4d_host_unproject(const float view[16], const float proj[16], int width, int height, float px, float py, float depth, float world3[3]) {
    const double nx = 2.0 * ((double)px + 0.5) / (double)width - 1.0, ny = 2.0 * ((double)py + 0.5) / (double)height - 1.0;
    const double zv = -(double)depth;
    auto P = [&](int c, int r) { return (double)proj[4 * c + r]; };
    // clip_k - n_k * clip_w = 0 (k = x, y):  a_k * xv + b_k * yv = -c_k
    const double ax = P(0, 0) - nx * P(0, 3), bx = P(1, 0) - nx * P(1, 3), cx = P(2, 0) * zv + P(3, 0) - nx * (P(2, 3) * zv + P(3, 3));
    const double ay = P(0, 1) - ny * P(0, 3), by = P(1, 1) - ny * P(1, 3), cy = P(2, 1) * zv + P(3, 1) - ny * (P(2, 3) * zv + P(3, 3));
    const double det = ax * by - bx * ay;
    const double xv = (-cx * by + bx * cy) / det, yv = (-ax * cy + cx * ay) / det;
    // world = view^-1 * (xv, yv, zv, 1)
    double m[4][8];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { m[r][c] = (double)view[4 * c + r]; m[r][4 + c] = r == c ? 1.0 : 0.0; }
    for (int k = 0; k < 4; ++k) {
        int piv = k;
        for (int r = k + 1; r < 4; ++r) if (std::fabs(m[r][k]) > std::fabs(m[piv][k])) piv = r;
        if (piv != k) for (int c = 0; c < 8; ++c) std::swap(m[k][c], m[piv][c]);
        const double inv = 1.0 / m[k][k];
        for (int c = 0; c < 8; ++c) m[k][c] *= inv;
        for (int r = 0; r < 4; ++r) if (r != k) { const double f = m[r][k]; for (int c = 0; c < 8; ++c) m[r][c] -= f * m[k][c]; }
    }
    const double v[4] = { xv, yv, zv, 1.0 };
    double w[4];
    for (int r = 0; r < 4; ++r) w[r] = m[r][4] * v[0] + m[r][5] * v[1] + m[r][6] * v[2] + m[r][7] * v[3];
    for (int k = 0; k < 3; ++k) world3[k] = (float)(w[k] / w[3]);
}

// Bounds of the depth keys (arithmetic contract): every GS4D_KEY_REF_INV_EUCLID key of a record inside the box lo[7]..hi[7] of
// (x, y, z, mu_t, velocity = sig[3].xyz), as a uint32 bit pattern, lies in [*bias, *bias + *span].  gs4d_keygen subtracts the bias inside the
// sort's digit extraction and sizes the sort by the span.
// The proof is monotonicity, not a margin: the key kernels (sort.hip k_keygen, preprocess.hip blend_key_4d) evaluate gs4d_key::ref_inv_euclid of
// csrc/depth_key.h in float32, and every one of its correctly rounded operations is monotone in each argument.  The same float32 operations applied to the
// ends of the box (interval arithmetic; the product takes the four corners) therefore bound every intermediate of every record, rounding
// included, whatever the size of the coordinates — and the ends overflow exactly where a record can, which leaves a bound of 0 (x = +-inf, key
// = 0) by itself.  Only 0 * inf makes a NaN, and only a non-finite ct makes an inf factor: then, and for non-finite arguments, nothing is claimed.
// No upper bound is claimed when the camera is inside or on the box (keys up to +inf).  Built with -ffp-contract=off like the kernels.
void gs4d_host_key_bounds(const float lo[7], const float hi[7], float t, const float cam[3], int key_mode, uint32_t* bias, uint32_t* span) {
    *bias = 0u; *span = 0xFFFFFFFFu;
    if (key_mode != GS4D_KEY_REF_INV_EUCLID) return;
    bool ok = std::isfinite(t) && std::isfinite(cam[0]) && std::isfinite(cam[1]) && std::isfinite(cam[2]);
    for (int k = 0; k < 7; ++k) ok = ok && std::isfinite(lo[k]) && std::isfinite(hi[k]) && lo[k] <= hi[k];
    const float ct_lo = t - hi[3], ct_hi = t - lo[3];
    if (!ok || !std::isfinite(ct_lo) || !std::isfinite(ct_hi)) return;
    float far2[3], near2[3];
    for (int ax = 0; ax < 3; ++ax) {
        const float v_lo = lo[4 + ax], v_hi = hi[4 + ax];
        const float p1 = v_lo * ct_lo, p2 = v_lo * ct_hi, p3 = v_hi * ct_lo, p4 = v_hi * ct_hi;
        const float m_lo = lo[ax] + std::min(std::min(p1, p2), std::min(p3, p4));
        const float m_hi = hi[ax] + std::max(std::max(p1, p2), std::max(p3, p4));
        const float d_lo = m_lo - cam[ax], d_hi = m_hi - cam[ax];
        const float far = std::max(std::fabs(d_lo), std::fabs(d_hi));
        const float near = d_lo > 0.0f ? d_lo : (d_hi < 0.0f ? -d_hi : 0.0f);
        far2[ax] = far * far; near2[ax] = near * near;
    }
    const float key_lo = 1.0f / std::sqrt((far2[0] + far2[1]) + far2[2]);
    const float n2 = (near2[0] + near2[1]) + near2[2];
    std::memcpy(bias, &key_lo, 4);
    if (n2 > 0.0f) {
        const float key_hi = 1.0f / std::sqrt(n2);
        uint32_t ubits; std::memcpy(&ubits, &key_hi, 4);
        if (ubits >= *bias) *span = ubits - *bias;
    }
}

// ---- Camera input model (Camera.cpp:90-99, 116-220) ----------------------------------------------------------------------
static Vec3 v3(const float* p) { return { p[0], p[1], p[2] }; }
static void put(float* p, Vec3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
static Vec3 add(Vec3 a, Vec3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
// glm::rotate(vec3 v, float angle, vec3 normal) = mat3(glm::rotate(mat4(1), angle, normal)) * v   (gtx/rotate_vector.inl:44-52,
// ext/matrix_transform.inl:18-46; with m = identity the 4x4 product leaves Rotate itself)
static Vec3 rotate_about(Vec3 v, float angle, Vec3 normal) {
    const float c = std::cos(angle), s = std::sin(angle);
    const Vec3 axis = unit(normal);
    const Vec3 temp = scale(axis, 1.0f - c);
    float R[3][3];
    R[0][0] = c + temp.x * axis.x;          R[0][1] = temp.x * axis.y + s * axis.z; R[0][2] = temp.x * axis.z - s * axis.y;
    R[1][0] = temp.y * axis.x - s * axis.z; R[1][1] = c + temp.y * axis.y;          R[1][2] = temp.y * axis.z + s * axis.x;
    R[2][0] = temp.z * axis.x + s * axis.y; R[2][1] = temp.z * axis.y - s * axis.x; R[2][2] = c + temp.z * axis.z;
    // Result[k] = m[0]*R[k][0] + m[1]*R[k][1] + m[2]*R[k][2] with m = identity: the products by 0 and 1 are exact, the sums add zeros
    float M[3][3];
    for (int k = 0; k < 3; ++k) for (int r = 0; r < 3; ++r) {
        const float e0 = (r == 0 ? 1.0f : 0.0f) * R[k][0], e1 = (r == 1 ? 1.0f : 0.0f) * R[k][1], e2 = (r == 2 ? 1.0f : 0.0f) * R[k][2];
        M[k][r] = e0 + e1 + e2;
    }
    return { M[0][0] * v.x + M[1][0] * v.y + M[2][0] * v.z, M[0][1] * v.x + M[1][1] * v.y + M[2][1] * v.z, M[0][2] * v.x + M[1][2] * v.y + M[2][2] * v.z };
}

void gs4d_host_camera_rotate(gs4d_camera_state* st, double mouseX, double mouseY) {
    if (st->fix_view) return;
    const double rotX = -(double)st->sensitivity * (mouseY - int((double)st->height / 2.0)) / (double)(st->height);
    const double rotY = -(double)st->sensitivity * (mouseX - int((double)st->width / 2.0)) / (double)(st->width);
    Vec3 o = v3(st->orientation), u = v3(st->up);
    if (!st->lock_x) o = rotate_about(o, (float)(rotX * 0.01745329251994329576923690768489), unit(cross(o, u)));
    const Vec3 side = unit(cross(u, o));
    u = unit(cross(o, side));
    if (!st->lock_y) o = rotate_about(o, (float)(rotY * 0.01745329251994329576923690768489), u);
    put(st->orientation, o); put(st->up, u);
}

void gs4d_host_camera_input(gs4d_camera_state* st, const gs4d_camera_input* in, int* recenter_cursor, int* hide_cursor) {
    if (recenter_cursor) *recenter_cursor = 0;
    if (hide_cursor) *hide_cursor = 0;
    if (in->imgui_active) return;
    const float currentSpeed = (in->keys & GS4D_CAMKEY_LSHIFT) ? st->fast_speed : st->speed;
    Vec3 p = v3(st->position), o = v3(st->orientation), u = v3(st->up);
    if (!st->fix_position) {
        if (in->keys & GS4D_CAMKEY_W) p = add(p, scale(o, currentSpeed));
        if (in->keys & GS4D_CAMKEY_S) p = add(p, scale(o, -currentSpeed));
        if (in->keys & GS4D_CAMKEY_A) { const Vec3 r = unit(cross(o, u)); const float k = -currentSpeed; p = add(p, { k * r.x, k * r.y, k * r.z }); }
        if (in->keys & GS4D_CAMKEY_D) { const Vec3 r = unit(cross(o, u)); p = add(p, { currentSpeed * r.x, currentSpeed * r.y, currentSpeed * r.z }); }
    }
    if (in->keys & GS4D_CAMKEY_E) u = rotate_about(u, 1.0f * 0.01745329251994329576923690768489f, o);
    if (in->keys & GS4D_CAMKEY_Q) u = rotate_about(u, -1.0f * 0.01745329251994329576923690768489f, o);
    if (in->keys & GS4D_CAMKEY_SPACE) p = add(p, { currentSpeed * u.x, currentSpeed * u.y, currentSpeed * u.z });
    if (in->keys & GS4D_CAMKEY_LCTRL) { const float k = -currentSpeed; p = add(p, { k * u.x, k * u.y, k * u.z }); }
    put(st->position, p); put(st->up, u);
    double mx = in->mouse_x, my = in->mouse_y;
    if ((in->keys & GS4D_CAMKEY_C) && !st->capture_mouse) {
        if (hide_cursor) *hide_cursor = 1;
        if (recenter_cursor) *recenter_cursor = 1;
        mx = (double)st->width / 2.0; my = (double)st->height / 2.0;
        st->first_capture = 0; st->capture_mouse = 1;
    }
    if (in->keys & GS4D_CAMKEY_ESC) st->capture_mouse = 0;
    if (st->capture_mouse) {
        if (!st->fix_view && recenter_cursor) *recenter_cursor = 1;
        gs4d_host_camera_rotate(st, mx, my);
    }
}

void gs4d_host_camera_look_at_point(gs4d_camera_state* st, const float point[3]) {
    const Vec3 o = unit(sub(v3(point), v3(st->position)));
    const Vec3 side = unit(cross(v3(st->up), o));
    put(st->orientation, o); put(st->up, unit(cross(o, side)));
}

void gs4d_host_camera_viewport(int width, int height, float out2[2]) {        // glm::normalize(glm::vec2(w, h)) = v * inversesqrt(dot(v, v))
    const float x = (float)width, y = (float)height;
    const float inv = 1.0f / std::sqrt(x * x + y * y);
    out2[0] = x * inv; out2[1] = y * inv;
}

void gs4d_host_camera_focal(float fov, int width, int height, float out2[2]) { // the reference passes DEGREES to tanf (Camera.cpp:97): reproduced
    const float d = (2.0f * tanf(fov * 0.5f));
    out2[0] = width / d; out2[1] = height / d;
}

void gs4d_host_quat_look_at(const float dir[3], const float up[3], float q_wxyz[4]) {
    const Vec3 d = unit(Vec3{ dir[0], dir[1], dir[2] });
    const Vec3 back = { -d.x, -d.y, -d.z };
    const Vec3 right = cross({ up[0], up[1], up[2] }, back);
    const Vec3 c0 = scale(right, 1.0f / std::sqrt(std::fmax(0.00001f, dot(right, right))));
    const Vec3 c1 = cross(back, c0);
    const M3 B = { { c0.x, c0.y, c0.z,  c1.x, c1.y, c1.z,  back.x, back.y, back.z } };
    const Quat q = gs4d_build::unit(quat_of(B));
    q_wxyz[0] = q.w; q_wxyz[1] = q.x; q_wxyz[2] = q.y; q_wxyz[3] = q.z;
}

void gs4d_host_splat3d_cov(const float q_wxyz[4], const float scale3[3], float cov9[9]) {
    const M3 g = gs4d_build::sigma3({ q_wxyz[0], q_wxyz[1], q_wxyz[2], q_wxyz[3] }, scale3);
    std::memcpy(cov9, g.a, sizeof g.a);
}

// Splat3D::GetSplatMesh / MakeMesh (Splat.h:433-473; vertex layout Geometry.h:37-42): the four 72-byte vertices of one splat's quad,
// {corner(2), position(3), colour(4), Sigma3(9, column-major)}, corners in the order the index buffer 0,2,1 / 2,0,3 expects (Geometry.h:44-50).
void gs4d_host_splat3d_mesh(const float pos3[3], const float q_wxyz[4], const float scale3[3], const float color4[4], float verts72[72]) {
    float cov[9];
    gs4d_host_splat3d_cov(q_wxyz, scale3, cov);
    static const float corner[4][2] = { { 0.5f, 0.5f }, { 0.5f, -0.5f }, { -0.5f, -0.5f }, { -0.5f, 0.5f } };
    for (int v = 0; v < 4; ++v) {
        float* o = verts72 + 18 * v;
        o[0] = corner[v][0]; o[1] = corner[v][1];
        std::memcpy(o + 2, pos3, 12);
        std::memcpy(o + 5, color4, 16);
        std::memcpy(o + 9, cov, 36);
    }
}

// Splat2D ctor + CalcAndSetSigma (Splat.h:551-582): Sigma^-1 of R S S^T R^T with R = (normalize(v0), normalize(v0.y, -v0.x)), S = diag(sqrt l0, sqrt l1)
void gs4d_host_splat2d_sigma_inv(const float v0[2], float l0, float l1, float sigma_inv4[4]) {
    const float s0 = sqrtf(l0), s1 = sqrtf(l1);
    auto norm2 = [](float x, float y, float* o) { const float inv = 1.0f / std::sqrt(x * x + y * y); o[0] = x * inv; o[1] = y * inv; };   // glm::normalize = v * inversesqrt(dot(v, v))
    float r0[2], r1[2];
    norm2(v0[0], v0[1], r0);
    norm2(v0[1], -v0[0], r1);
    // column-major 2x2: m[c][r]; glm mat2 * mat2 (type_mat2x2.inl:453-460)
    struct M2 { float m[2][2]; };
    auto mul = [](const M2& a, const M2& b) { M2 c;
        c.m[0][0] = a.m[0][0] * b.m[0][0] + a.m[1][0] * b.m[0][1]; c.m[0][1] = a.m[0][1] * b.m[0][0] + a.m[1][1] * b.m[0][1];
        c.m[1][0] = a.m[0][0] * b.m[1][0] + a.m[1][0] * b.m[1][1]; c.m[1][1] = a.m[0][1] * b.m[1][0] + a.m[1][1] * b.m[1][1]; return c; };
    auto tr = [](const M2& a) { M2 c; c.m[0][0] = a.m[0][0]; c.m[0][1] = a.m[1][0]; c.m[1][0] = a.m[0][1]; c.m[1][1] = a.m[1][1]; return c; };
    const M2 S = { { { s0, 0.0f }, { 0.0f, s1 } } }, R = { { { r0[0], r0[1] }, { r1[0], r1[1] } } };
    const M2 sig = mul(mul(mul(R, S), tr(S)), tr(R));
    const float ood = 1.0f / (sig.m[0][0] * sig.m[1][1] - sig.m[1][0] * sig.m[0][1]);        // glm::inverse (func_matrix.inl:303-317)
    sigma_inv4[0] = sig.m[1][1] * ood; sigma_inv4[1] = -sig.m[0][1] * ood; sigma_inv4[2] = -sig.m[1][0] * ood; sigma_inv4[3] = sig.m[0][0] * ood;
}

// One 48-byte record of the Gaussians2D scene (Scenes.h:1490-1496, struct :1447-1452): {x, y, 0, 0 | r, g, b, 1 | R S S R^T} with
// R = {cosf a, -sinf a, sinf a, cos a} (`cos` on a float picks the float overload, here as under MSVC: the fixtures confirm it).
void gs4d_host_gaussians2d_record(float angle, float s0, float s1, float px, float py, const float rgb[3], float rec12[12]) {
    struct M2 { float m[2][2]; };
    auto mul = [](const M2& a, const M2& b) { M2 c;
        c.m[0][0] = a.m[0][0] * b.m[0][0] + a.m[1][0] * b.m[0][1]; c.m[0][1] = a.m[0][1] * b.m[0][0] + a.m[1][1] * b.m[0][1];
        c.m[1][0] = a.m[0][0] * b.m[1][0] + a.m[1][0] * b.m[1][1]; c.m[1][1] = a.m[0][1] * b.m[1][0] + a.m[1][1] * b.m[1][1]; return c; };
    auto tr = [](const M2& a) { M2 c; c.m[0][0] = a.m[0][0]; c.m[0][1] = a.m[1][0]; c.m[1][0] = a.m[0][1]; c.m[1][1] = a.m[1][1]; return c; };
    const M2 R = { { { cosf(angle), -sinf(angle) }, { sinf(angle), std::cos(angle) } } }, S = { { { s0, 0.0f }, { 0.0f, s1 } } };
    const M2 g = mul(mul(mul(R, S), S), tr(R));
    rec12[0] = px; rec12[1] = py; rec12[2] = 0.0f; rec12[3] = 0.0f;
    rec12[4] = rgb[0]; rec12[5] = rgb[1]; rec12[6] = rgb[2]; rec12[7] = 1.0f;
    rec12[8] = g.m[0][0]; rec12[9] = g.m[0][1]; rec12[10] = g.m[1][0]; rec12[11] = g.m[1][1];
}

float gs4d_host_time_variance(float lifetime, float fade) {
    // Splat.h:139: `log(fadeof)` on a float is the float overload; the -2.0 factor promotes the quotient to double
    const double denom = (fade == 0.5f) ? (double)1.3862943611198906f : -2.0 * (double)std::log(fade);
    return (float)((double)(lifetime * lifetime) / denom);
}

void gs4d_host_time_variances(size_t n, const float* lifetime, const float* fade, float* out) {
    for (size_t i = 0; i < n; ++i) out[i] = gs4d_host_time_variance(lifetime[i], fade[i]);
}

// The builders below are calls of csrc/build_record.h, the text the kernels of gs4d_build_records compile; the time variance stays here
void gs4d_host_splat4d_cov(const float q_wxyz[4], const float scale3[3], float lifetime, float fade, const float dir[3], float cov16[16]) {
    gs4d_build::cov_4d_vel(q_wxyz, scale3, dir, gs4d_host_time_variance(lifetime, fade), cov16);
}

void gs4d_host_splat4d_cov2q(const float q0_wxyz[4], const float q1_wxyz[4], const float scale4[4], float cov16[16]) {
    gs4d_build::cov_4d_2q(q0_wxyz, q1_wxyz, scale4, cov16);
}

void gs4d_host_build_records_3d(size_t n, const float* pos3, const float* q_wxyz, const float* scale3, const float* rgba, float* rec) {
    for (size_t i = 0; i < n; ++i) gs4d_build::record_3d(pos3 + 3 * i, q_wxyz + 4 * i, scale3 + 3 * i, rgba + 4 * i, rec + 24 * i);
}

void gs4d_host_build_records_4d(size_t n, const float* pos4, const float* q_wxyz, const float* scale3, const float* lifetime, const float* fade,
                                const float* dir3, const float* rgba, float* rec) {
    for (size_t i = 0; i < n; ++i)
        gs4d_build::record_4d_vel(pos4 + 4 * i, q_wxyz + 4 * i, scale3 + 3 * i, dir3 + 3 * i, gs4d_host_time_variance(lifetime[i], fade[i]), rgba + 4 * i, rec + 24 * i);
}

void gs4d_host_build_records_4d_tvar(size_t n, const float* pos4, const float* q_wxyz, const float* scale3, const float* dir3, const float* tvar,
                                     const float* rgba, float* rec) {
    for (size_t i = 0; i < n; ++i) gs4d_build::record_4d_vel(pos4 + 4 * i, q_wxyz + 4 * i, scale3 + 3 * i, dir3 + 3 * i, tvar[i], rgba + 4 * i, rec + 24 * i);
}

void gs4d_host_build_records_4d_2q(size_t n, const float* pos4, const float* q0_wxyz, const float* q1_wxyz, const float* scale4, const float* rgba, float* rec) {
    for (size_t i = 0; i < n; ++i) gs4d_build::record_4d_2q(pos4 + 4 * i, q0_wxyz + 4 * i, q1_wxyz + 4 * i, scale4 + 4 * i, rgba + 4 * i, rec + 24 * i);
}

// The definition of gs4d_decompose_records (gs4d.h) is csrc/decompose_record.h: the builders above, backwards.  A destination that is null is not
// wanted; the eigen-solve is left out when neither q_wxyz nor scale3 is.  A form the device call would refuse writes nothing; dir3 and tvar are not
// written in the 3D form.
extern "C++" {
template <int FORM, bool SOLVE>
static void decompose_rows(size_t n, const float* rec, float* pos, float* q, float* scale3, float* rgba, float* dir3, float* tvar) {
    constexpr size_t pw = FORM == GS4D_PARAMS_3D ? 3 : 4;
    for (size_t i = 0; i < n; ++i) {
        gs4d_decompose::Splat s;
        gs4d_decompose::record<FORM, SOLVE>(rec + 24 * i, s);
        if (pos) std::memcpy(pos + pw * i, s.pos, 4 * pw);
        if (SOLVE && q) std::memcpy(q + 4 * i, s.q, 16);
        if (SOLVE && scale3) std::memcpy(scale3 + 3 * i, s.s, 12);
        if (rgba) std::memcpy(rgba + 4 * i, s.rgba, 16);
        if (FORM != GS4D_PARAMS_3D && dir3) std::memcpy(dir3 + 3 * i, s.dir, 12);
        if (FORM != GS4D_PARAMS_3D && tvar) tvar[i] = s.tvar;
    }
}
}
void gs4d_host_decompose_records(size_t n, const float* rec, uint32_t form, float* pos, float* q_wxyz, float* scale3, float* rgba, float* dir3, float* tvar) {
    if (form != GS4D_PARAMS_3D && form != GS4D_PARAMS_4D_VEL) return;
    const bool vel = form == GS4D_PARAMS_4D_VEL, solve = q_wxyz || scale3;
    (vel ? (solve ? &decompose_rows<GS4D_PARAMS_4D_VEL, true> : &decompose_rows<GS4D_PARAMS_4D_VEL, false>)
         : (solve ? &decompose_rows<GS4D_PARAMS_3D, true> : &decompose_rows<GS4D_PARAMS_3D, false>))(n, rec, pos, q_wxyz, scale3, rgba, dir3, tvar);
}

// The definition of gs4d_transform_records (gs4d.h) is csrc/transform_record.h: mean L p + o, covariance (L Sigma) L^T as two full mat4 products, rgba copied
void gs4d_host_transform_records(size_t n, const float* rec, const gs4d_affine4* xf, float* out) {
    for (size_t i = 0; i < n; ++i) gs4d_transform::record(xf->l, xf->o, rec + 24 * i, out + 24 * i);
}

// The definition of gs4d_pose_records (gs4d.h) is csrc/pose_record.h: the record under the row its bind row names, under the blend of up to four, or
// copied.  A form or a stride the device call would refuse writes nothing.
void gs4d_host_pose_records(size_t n, const float* rec, const gs4d_affine4* xf, size_t m, const void* bind, uint32_t form, size_t bind_stride, float* out) {
    if (form == GS4D_POSE_INDEX ? (bind_stride < 4 || bind_stride % 4 != 0) : form == GS4D_POSE_BLEND4 ? (bind_stride < 32 || bind_stride % 16 != 0) : true) return;
    const unsigned int rows_m = m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned int)m;
    const auto rows = [xf](unsigned int j, float r[20]) { std::memcpy(r, &xf[j], sizeof(gs4d_affine4)); };
    for (size_t i = 0; i < n; ++i) {
        const unsigned char* const row = (const unsigned char*)bind + i * bind_stride;
        if (form == GS4D_POSE_INDEX) {
            uint32_t j;
            std::memcpy(&j, row, 4);
            gs4d_pose::index(rows, rows_m, j, rec + 24 * i, out + 24 * i);
        } else {
            unsigned int j[4];
            float w[4];
            std::memcpy(j, row, 16);
            std::memcpy(w, row + 16, 16);
            gs4d_pose::blend(rows, rows_m, j, w, rec + 24 * i, out + 24 * i);
        }
    }
}

// The definition of gs4d_rotate_sh (gs4d.h) is csrc/sh_rotate_record.h: the frame of a map's spatial block, the band matrices of that frame, and the
// row under them — or the row copied, where it names no map or its map does not rotate.  Arguments the device call would refuse (the scalar rules
// of csrc/sh_rotate_operands.h) write nothing.
int gs4d_host_sh_rotation(const float l[16], float d[84]) {
    return gs4d_shrot::rotation<3>(l, d) ? 1 : 0;
}
} // extern "C"
namespace {
template <int DEGREE>
void rotate_sh_rows(size_t n, const unsigned char* rows, size_t stride, const gs4d_affine4* xf, size_t m, const unsigned char* bind, uint32_t form, size_t bind_stride,
                    unsigned char* out) {
    constexpr size_t used = 12u * (size_t)gs4d_shrot::coeffs(DEGREE);
    const unsigned int rows_m = (unsigned int)m;
    const auto table = [xf](unsigned int j, float r[20]) { std::memcpy(r, &xf[j], sizeof(gs4d_affine4)); };
    const size_t instances = form == GS4D_SH_EACH ? m : 1;
    for (size_t inst = 0; inst < instances; ++inst)
        for (size_t i = 0; i < n; ++i) {
            const unsigned char* const row = rows + i * stride;
            unsigned char* const to = out + (inst * n + i) * stride;
            std::memcpy(to, row, stride);
            if (DEGREE == 0) continue;
            float a[20];
            bool mapped;
            if (form == GS4D_SH_EACH) {
                table((unsigned int)inst, a);
                mapped = true;
            } else if (form == GS4D_POSE_INDEX) {
                uint32_t j;
                std::memcpy(&j, bind + i * bind_stride, 4);
                mapped = gs4d_shrot::index_map(table, rows_m, j, a);
            } else {
                unsigned int j[4];
                float w[4];
                std::memcpy(j, bind + i * bind_stride, 16);
                std::memcpy(w, bind + i * bind_stride + 16, 16);
                mapped = gs4d_pose::blend4(table, rows_m, j, w, a);
            }
            if (!mapped) continue;
            float c[used / 4];
            std::memcpy(c, row, used);
            if (gs4d_shrot::coefficients<DEGREE>(a, c)) std::memcpy(to + 12, c + 3, used - 12);      // (words 0..2 are the copy's)
        }
}
}
extern "C" {
void gs4d_host_rotate_sh(size_t n, const void* rows, size_t stride, int degree, const gs4d_affine4* xf, size_t m, const void* bind, uint32_t form, size_t bind_stride,
                         void* out) {
    if (gs4d::rotate_sh_fault(n, stride, degree, m, bind != nullptr, form, bind_stride, 0)) return;
    (degree == 0 ? &rotate_sh_rows<0> : degree == 1 ? &rotate_sh_rows<1> : degree == 2 ? &rotate_sh_rows<2> : &rotate_sh_rows<3>)(
        n, (const unsigned char*)rows, stride, xf, m, (const unsigned char*)bind, form, bind_stride, (unsigned char*)out);
}

// The definitions of gs4d_shade_sh_t and gs4d_collapse_sh (gs4d.h) are csrc/sh_time_record.h: the weights of the time blocks from the record's mu_t,
// the effective row they fold a 4D row into, and gs4d_shade_sh's colour of a record from that row.  Arguments the device calls would refuse write nothing.
void gs4d_host_sh_time_weights(const gs4d_sh_time* q, float mu_t, float w[2], int* mask) {
    w[0] = w[1] = 0.0f;
    *mask = 0;
    if (!q || q->degree_t < 0 || q->degree_t > gs4d_sht::MAX_DEGREE_T) return;
    *mask = (int)gs4d_sht::weights(q->degree_t, q->t, q->inv_period, mu_t, w);
}
} // extern "C"
namespace {
// e <- the effective row of row i for record i
void effective_row_at(size_t i, const float* rec, const unsigned char* sh, size_t sh_stride, const gs4d_sh_time& q, float e[48]) {
    float row[48 * 3], w[2];
    std::memcpy(row, sh + i * sh_stride, 4u * gs4d_sht::row_words_t(q.degree, q.degree_t));
    const uint32_t mask = gs4d_sht::weights(q.degree_t, q.t, q.inv_period, rec[24 * i + 3], w);
    gs4d_sht::effective_row(q.degree, q.degree_t, row, w, mask, e);
}
}
extern "C" {
void gs4d_host_collapse_sh(size_t n, const float* rec, const void* sh, size_t sh_stride, const gs4d_sh_time* q, void* dst, size_t dst_stride) {
    if (!q || gs4d_sht::query_fault(n, q->degree, q->degree_t, q->reserved, sh_stride) || gs4d_sht::dst_stride_fault(q->degree, dst_stride)) return;
    const size_t used = 4u * gs4d_sht::row_words(q->degree);
    for (size_t i = 0; i < n; ++i) {
        float e[48];
        effective_row_at(i, rec, (const unsigned char*)sh, sh_stride, *q, e);
        unsigned char* const to = (unsigned char*)dst + i * dst_stride;
        std::memcpy(to, e, used);
        std::memset(to + used, 0, dst_stride - used);
    }
}

void gs4d_host_shade_sh_t(size_t n, float* rec, const void* sh, size_t sh_stride, const gs4d_sh_time* q) {
    if (!q || gs4d_sht::query_fault(n, q->degree, q->degree_t, q->reserved, sh_stride)) return;
    for (size_t i = 0; i < n; ++i) {
        float e[48], *const r = rec + 24 * i;
        effective_row_at(i, rec, (const unsigned char*)sh, sh_stride, *q, e);
        const float* const cam = q->cam_pos;
        switch (q->degree) {
        case 0: gs4d_sht::colour<0>(r, r + 20, q->t, cam[0], cam[1], cam[2], e, r + 4); break;
        case 1: gs4d_sht::colour<1>(r, r + 20, q->t, cam[0], cam[1], cam[2], e, r + 4); break;
        case 2: gs4d_sht::colour<2>(r, r + 20, q->t, cam[0], cam[1], cam[2], e, r + 4); break;
        default: gs4d_sht::colour<3>(r, r + 20, q->t, cam[0], cam[1], cam[2], e, r + 4); break;
        }
    }
}

// The definition of gs4d_warp_records (gs4d.h) is csrc/warp_record.h: the record through the lattice's map linearised at its centre, or copied.  A
// lattice the device call would refuse writes nothing.
void gs4d_host_warp_records(size_t n, const float* rec, const float* nodes4, const gs4d_lattice* lat, float* out) {
    if (!lat || !gs4d_warp::node_count(lat->dims, lat->clamp, lat->pad)) return;
    const auto nodes = [nodes4](unsigned int j, float v[4]) { std::memcpy(v, nodes4 + 4 * (size_t)j, 16); };
    for (size_t i = 0; i < n; ++i) {
        if (lat->dims[3] >= 2u) gs4d_warp::record<true>(nodes, lat->lo, lat->inv, lat->dims, lat->clamp, rec + 24 * i, out + 24 * i);
        else gs4d_warp::record<false>(nodes, lat->lo, lat->inv, lat->dims, lat->clamp, rec + 24 * i, out + 24 * i);
    }
}

// The definition of gs4d_slice_records (gs4d.h) is csrc/slice_record.h: the draw's time conditioning at q->t, baked into the record
void gs4d_host_slice_records(size_t n, const float* rec, const gs4d_slice* q, float* out) {
    for (size_t i = 0; i < n; ++i) gs4d_slicing::record(q->t, q->min_opacity, q->mu_t_out, q->s44_out, rec + 24 * i, out + 24 * i);
}

// ---- what the definitions that select by, or add to, a record-statistics table share ----
namespace {
constexpr uint32_t ONE_BITS = 0x3F800000u;                  // the bits of 1.0f: the wmax of a fragment of weight 1
// a rule the device calls take: known flags, a zero reserved field
bool rule_ok(const gs4d_keep_rule* rule) { return rule->reserved == 0u && (rule->flags & ~(uint32_t)GS4D_KEEP_INVERT) == 0u; }
// whether a row passes the rule: the predicate of gs4d_compact_records (the device's keep_row)
bool keeps(const gs4d_record_stat& s, const gs4d_keep_rule* rule) {
    return (s.pixels >= rule->min_pixels && s.wmax >= rule->min_wmax && s.wsum >= rule->min_wsum) != ((rule->flags & (uint32_t)GS4D_KEEP_INVERT) != 0u);
}
// c fragments of weight 1 into a row (the device's add_fragments)
void add_fragments(gs4d_record_stat& s, uint32_t c, uint32_t wmax_bits) { s.pixels += c; s.wmax = std::max(s.wmax, wmax_bits); s.wsum += (uint64_t)c << 24; }
// What the three grid definitions start from: the centres at time t, who takes part under the GS4D_NB_* skips (takes_part of
// csrc/neighbour_query.h), and who is a source — it takes part and its row of `source` passes the rule (source == null: every such record).
struct Centres {
    std::vector<float> m;
    std::vector<uint8_t> part, src;
    Centres(size_t n, const float* rec, float t, uint32_t skips, const gs4d_record_stat* source, const gs4d_keep_rule* rule) : m(3 * n), part(n), src(n) {
        for (size_t i = 0; i < n; ++i) {
            const float* p = rec + 24 * i;
            const gs4d_neighbour::Fields r{ { p[0], p[1], p[2] }, p[3], p[7], { p[20], p[21], p[22] }, p[23] };
            part[i] = gs4d_neighbour::takes_part(t, skips, r, &m[3 * i]);
            src[i] = part[i] && (!source || keeps(source[i], rule));
        }
    }
};
}

// The definition of gs4d_edit_colours (gs4d.h), in place: the selection by the rule of gs4d_compact_records, then the edit per channel of the mask.
// This file is built with -ffp-contract=off: the product and the sums of MUL and LERP are rounded one by one.  SET and COPY move bits.  An edit
// the device call would refuse (unknown op, channels outside 1 .. 15) edits nothing.
void gs4d_host_edit_colours(size_t n, float* rec, const gs4d_record_stat* stats, const gs4d_keep_rule* rule, const gs4d_colour_edit* edit, const float* from) {
    if (!edit || edit->op > (uint32_t)GS4D_EDIT_COPY || edit->channels == 0u || edit->channels > 15u) return;
    if (edit->op == (uint32_t)GS4D_EDIT_COPY && !from) return;
    if (stats && !rule) return;
    for (size_t i = 0; i < n; ++i) {
        if (stats && !keeps(stats[i], rule)) continue;
        for (uint32_t ch = 0; ch < 4u; ++ch) {
            if (!((edit->channels >> ch) & 1u)) continue;
            float* const c = rec + 24 * i + 4 + ch;
            switch (edit->op) {
                case GS4D_EDIT_SET: std::memcpy(c, &edit->value[ch], 4); break;
                case GS4D_EDIT_MUL: *c = *c * edit->value[ch]; break;
                case GS4D_EDIT_LERP: { const float d = edit->value[ch] - *c; const float step = edit->amount * d; *c = *c + step; break; }
                default: std::memcpy(c, from + 24 * i + 4 + ch, 4); break;
            }
        }
    }
}

// The definition of gs4d_count_centres (gs4d.h), in place on the table: whether record i takes part is the text of csrc/centre_query.h, which the
// kernel compiles too (this file is built with -ffp-contract=off); then the row.  A query the device call would refuse changes nothing.
void gs4d_host_count_centres(size_t n, const float* rec, const gs4d_centre_query* q, int width, int height, const uint8_t* mask, gs4d_record_stat* stats) {
    const uint32_t known = GS4D_CQ_BOX | GS4D_CQ_SPHERE | GS4D_CQ_SCREEN | GS4D_CQ_FRAME | GS4D_CQ_SKIP_HIDDEN | GS4D_CQ_SKIP_DEAD;
    if (!q || (q->tests & ~known) != 0u || q->op > (uint32_t)GS4D_CQ_REMOVE || q->reserved != 0u) return;
    const bool screen = (q->tests & (uint32_t)GS4D_CQ_SCREEN) != 0u;
    if (mask && !screen) return;
    if (screen && (q->x < 0 || q->y < 0 || q->w <= 0 || q->h <= 0 || q->w > width - q->x || q->h > height - q->y)) return;
    const float hw = (float)width * 0.5f, hh = (float)height * 0.5f;
    for (size_t i = 0; i < n; ++i) {
        const float* p = rec + 24 * i;
        const gs4d_centre::Fields r{ { p[0], p[1], p[2] }, p[3], p[7], { p[20], p[21], p[22] }, p[23] };
        if (!gs4d_centre::takes_part(*q, hw, hh, r, mask)) continue;
        gs4d_record_stat& s = stats[i];
        if (q->op == (uint32_t)GS4D_CQ_ADD) add_fragments(s, 1u, ONE_BITS);
        else s = gs4d_record_stat{ 0u, 0u, 0ull };
    }
}

// The definition of gs4d_measure_records (gs4d.h): what a selected record adds is the text of csrc/measure_record.h, which the kernels compile too
// (this file is built with -ffp-contract=off) — one pass for the counts and the keyed extrema, one for the cells once the box is known.  A query the
// device call would refuse gives the empty measurement.
void gs4d_host_measure_records(size_t n, const float* rec, const gs4d_measure_query* q, const gs4d_record_stat* stats, const gs4d_keep_rule* rule, gs4d_measure* out) {
    namespace ms = gs4d_measure_rec;
    uint32_t row[ms::ROW_WORDS];
    for (int w = 0; w < ms::ROW_WORDS; ++w) row[w] = ms::row_empty(w);
    const uint32_t known = GS4D_MS_SKIP_HIDDEN | GS4D_MS_SKIP_DEAD;
    const bool valid = q && (q->flags & ~known) == 0u && q->reserved[0] == 0u && q->reserved[1] == 0u && !(stats && !rule);
    auto selected = [&](size_t i) { return !stats || keeps(stats[i], rule); };
    auto fields = [&](size_t i) {
        const float* p = rec + 24 * i;
        return ms::Fields{ { { p[0], p[1], p[2] }, p[3], p[7], { p[20], p[21], p[22] }, p[23] }, { p[8], p[13], p[18] } };
    };
    if (valid) for (size_t i = 0; i < n; ++i) if (selected(i)) ms::add_record(q->t, q->flags, fields(i), row);
    uint32_t words[ms::ROW_WORDS];
    for (int w = 0; w < ms::ROW_WORDS; ++w) words[w] = ms::row_word(w, row[w]);
    std::memset(out, 0, sizeof *out);
    std::memcpy(out, words, sizeof words);
    if (!valid || out->count == 0u) return;
    for (size_t i = 0; i < n; ++i) {
        if (!selected(i)) continue;
        float m[3];
        if (ms::place(q->t, q->flags, fields(i).c, m) != ms::MEASURED) continue;
        for (int a = 0; a < 3; ++a) out->cell_sum[a] += ms::cell(m[a], out->lo[a], out->hi[a]);
    }
}

// The definition of gs4d_count_neighbours (gs4d.h), in place on the table: the brute-force double loop over the text of csrc/neighbour_query.h,
// which the kernels compile too (this file is built with -ffp-contract=off), with the early exit at cap; then the row.  No search structure: this
// is what the device's structure has to reproduce.  A query the device call would refuse changes nothing.
void gs4d_host_count_neighbours(size_t n, const float* rec, const gs4d_neighbour_query* q, const gs4d_record_stat* source, const gs4d_keep_rule* rule,
                                gs4d_record_stat* stats) {
    namespace nb = gs4d_neighbour;
    if (!q || !nb::query_ok(*q) || (source && !rule)) return;
    if (source && !rule_ok(rule)) return;
    const bool self = (q->flags & (uint32_t)GS4D_NB_COUNT_SELF) != 0u;
    const float rr = q->radius * q->radius;
    const Centres g(n, rec, q->t, q->flags, source, rule);
    for (size_t i = 0; i < n; ++i) {
        if (!g.part[i]) continue;
        uint32_t c = 0;
        for (size_t j = 0; j < n && c < q->cap; ++j)
            if (g.src[j] && (j != i || self) && nb::near(&g.m[3 * i], &g.m[3 * j], rr)) ++c;
        if (c != 0u) add_fragments(stats[i], c, ONE_BITS);
    }
}

// The definition of gs4d_label_components (gs4d.h): who is a member (takes_part of csrc/neighbour_query.h and the predicate of gs4d_edit_colours), the
// brute-force double loop over every pair of members with `near`, and the union–find of csrc/component_union.h — the text the kernels compile — run
// sequentially on plain words; then the labels and, with a table, the rows.  No search structure.  A query the device call would refuse changes
// nothing.
namespace {
struct PlainParents {
    uint32_t* p;
    uint32_t load(uint32_t x) const { return p[x]; }
    bool cas(uint32_t x, uint32_t is, uint32_t to) { if (p[x] != is) return false; p[x] = to; return true; }
    void lower(uint32_t x, uint32_t v) { if (v < p[x]) p[x] = v; }
};
}
void gs4d_host_label_components(size_t n, const float* rec, const gs4d_component_query* q, const gs4d_record_stat* source, const gs4d_keep_rule* rule,
                                uint32_t* labels, gs4d_record_stat* stats) {
    namespace nb = gs4d_neighbour;
    if (!q || n >= 0xFFFFFFFFull || (source && !rule)) return;
    const gs4d_neighbour_query as_nb{ q->t, q->radius, q->cap, q->flags, { q->reserved[0], q->reserved[1], q->reserved[2], q->reserved[3] } };
    if ((q->flags & ~(uint32_t)(GS4D_CC_SKIP_HIDDEN | GS4D_CC_SKIP_DEAD)) != 0u || !nb::query_ok(as_nb)) return;
    if (source && !rule_ok(rule)) return;
    const float rr = q->radius * q->radius;
    const Centres g(n, rec, q->t, q->flags, source, rule);
    const std::vector<float>& m = g.m;
    const std::vector<uint8_t>& member = g.src;                // a member is what the other two calls name a source
    std::vector<uint32_t> parent(n);
    for (size_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    PlainParents mem{ parent.data() };
    for (size_t i = 0; i < n; ++i) {
        if (!member[i]) continue;
        for (size_t j = 0; j < i; ++j)
            if (member[j] && nb::near(&m[3 * i], &m[3 * j], rr)) (void)gs4d_union::unite(mem, (uint32_t)i, (uint32_t)j, (uint32_t)n);
    }
    std::vector<uint32_t> size(n, 0u);
    for (size_t i = 0; i < n; ++i) {
        labels[i] = member[i] ? gs4d_union::find(mem, (uint32_t)i, (uint32_t)n) : (uint32_t)GS4D_ID_NONE;
        if (member[i]) ++size[labels[i]];
    }
    if (!stats) return;
    for (size_t i = 0; i < n; ++i) {
        if (!member[i]) continue;
        add_fragments(stats[i], std::min(q->cap, size[labels[i]]), ONE_BITS);
    }
}

// The definition of gs4d_count_labels (gs4d.h), in place on the table: the labels of the seeds, then one fragment for every record whose label is
// one of them.  A word >= n is no label.
void gs4d_host_count_labels(size_t n, const uint32_t* labels, const gs4d_record_stat* seeds, const gs4d_keep_rule* rule, gs4d_record_stat* stats) {
    if (!rule || !rule_ok(rule)) return;
    std::vector<uint8_t> hit(n, 0);
    for (size_t j = 0; j < n; ++j)
        if (labels[j] < n && keeps(seeds[j], rule)) hit[labels[j]] = 1;
    for (size_t i = 0; i < n; ++i)
        if (labels[i] < n && hit[labels[i]]) add_fragments(stats[i], 1u, ONE_BITS);
}

// The definition of gs4d_cell_labels (gs4d.h) is cell_label of csrc/merge_record.h
void gs4d_host_cell_labels(size_t n, const float* rec, const gs4d_cell_grid* grid, uint32_t* labels) {
    if (!grid || !gs4d_merge::grid_ok(grid->edge, grid->dims, grid->reserved)) return;
    for (size_t i = 0; i < n; ++i) labels[i] = gs4d_merge::cell_label(grid->lo, grid->edge, grid->dims, rec + 24 * i);
}

// The definition of gs4d_merge_records (gs4d.h) over the text of csrc/merge_record.h, which the kernels compile too (this file is built with
// -ffp-contract=off): the members, a stable sort of them by label, and per run of equal labels either the member itself or the eight interleaved
// slots, their fixed tree and the moments.  One thread, one loop.
void gs4d_host_merge_records(size_t n, const float* rec, const uint32_t* labels, const gs4d_merge_query* q, const gs4d_record_stat* stats,
                             const gs4d_keep_rule* rule, float* out, gs4d_merge_group* groups, uint32_t* member_group, gs4d_merge_count* count) {
    namespace mg = gs4d_merge;
    if (!q || !(mg::finite(q->alpha_max) && q->alpha_max > 0.0f) || q->flags != 0u || q->reserved[0] != 0u || q->reserved[1] != 0u) return;
    if (n >= 0xFFFFFFFFull || (stats != nullptr) != (rule != nullptr) || (rule && !rule_ok(rule))) return;
    std::vector<uint32_t> member;
    for (size_t i = 0; i < n; ++i) {
        float a;
        const bool is = labels[i] != mg::NONE && (!stats || keeps(stats[i], rule)) && mg::member_mass(rec + 24 * i, a);
        if (is) member.push_back((uint32_t)i);
        if (member_group) member_group[i] = mg::NONE;
    }
    std::stable_sort(member.begin(), member.end(), [labels](uint32_t x, uint32_t y) { return labels[x] < labels[y]; });
    uint32_t g = 0;
    for (size_t first = 0, end; first < member.size(); first = end, ++g) {
        const uint32_t label = labels[member[first]];
        for (end = first + 1; end < member.size() && labels[member[end]] == label; ++end) {}
        float* const o = out + 24 * (size_t)g;
        if (end - first == 1) {
            std::memcpy(o, rec + 24 * (size_t)member[first], 96);
        } else {
            const float* const origin = rec + 24 * (size_t)member[first];
            mg::Sums slot[mg::SLOTS];
            for (int s = 0; s < mg::SLOTS; ++s) mg::clear(slot[s]);
            for (size_t k = first; k < end; ++k) {
                const float* const r = rec + 24 * (size_t)member[k];
                float a;
                (void)mg::member_mass(r, a);
                mg::add_member(slot[(k - first) % mg::SLOTS], origin, a, r);
            }
            mg::join_slots(slot);
            mg::finish(slot[0], origin, q->alpha_max, o);
        }
        if (groups) groups[g] = gs4d_merge_group{ label, (uint32_t)(end - first), member[first], 0u };
        if (member_group) for (size_t k = first; k < end; ++k) member_group[member[k]] = g;
    }
    *count = gs4d_merge_count{ g, g, (uint32_t)member.size(), (uint32_t)(n - member.size()) };
}

// The definition of gs4d_merge_rows (gs4d.h) is host_merge_rows of csrc/merge_rows_record.h, whose word functions the kernels compile too
void gs4d_host_merge_rows(size_t n, const float* rec, const uint32_t* member_group, const void* rows, const gs4d_rows_query* q, void* dst, size_t dst_first,
                          size_t capacity, gs4d_merge_count* count) {
    static_assert(sizeof(gs4d_merge_count) == 4 * sizeof(uint32_t), "the count is four words");
    if (!q) return;
    gs4d_rows::host_merge_rows(n, rec, member_group, rows, q->stride, q->width, q->flags, q->reserved, dst, dst_first, capacity, &count->groups);
}

// The definition of gs4d_lod_cut (gs4d.h) over the text of csrc/lod_query.h, which the kernel compiles too (this file is built with
// -ffp-contract=off): the levels from the top down, one state per node, then the DRAW nodes in ascending index.  A query the device call would
// refuse writes nothing.
void gs4d_host_lod_cut(size_t n, const float* rec, const uint32_t* parent, const gs4d_lod_query* q, float* dst, uint32_t* cut_index,
                       gs4d_record_stat* stats, gs4d_lod_count* count, size_t capacity) {
    namespace lod = gs4d_lod;
    if (!q || !lod::query_ok(*q, n)) return;
    const lod::View view = lod::view_of(*q);
    std::vector<uint8_t> state(n, (uint8_t)lod::STOP);
    uint32_t tested = 0, drawn = 0, drawn_leaves = 0;
    for (int k = (int)q->levels - 1; k >= 0; --k) {
        const uint32_t next_first = q->level_first[k + 1];
        for (size_t i = q->level_first[k]; i < next_first; ++i) {
            const uint32_t p = parent[i];
            if (lod::is_child(p, next_first, (uint32_t)n) && state[p] != lod::DESCEND) continue;      // STOP: nothing of its record is looked at
            ++tested;
            const bool leaf = i < q->level_first[1];
            state[i] = lod::tested_state(leaf, !leaf && lod::fine(view, rec + 24 * i));
            if (state[i] == lod::DRAW && leaf) ++drawn_leaves;
        }
    }
    for (size_t i = 0; i < n; ++i) {
        if (state[i] != lod::DRAW) continue;
        if (drawn < capacity) {
            if (dst) std::memcpy(dst + 24 * (size_t)drawn, rec + 24 * i, 96);
            if (cut_index) cut_index[drawn] = (uint32_t)i;
        }
        if (stats) add_fragments(stats[i], 1u, ONE_BITS);
        ++drawn;
    }
    *count = gs4d_lod_count{ drawn, (uint32_t)(drawn < capacity ? drawn : capacity), tested, drawn_leaves };
}

// The definition of gs4d_nearest_neighbours (gs4d.h): the brute-force double loop over the texts of csrc/neighbour_query.h and
// csrc/nearest_query.h, which the kernels compile too (this file is built with -ffp-contract=off) — every source that is near goes into the sorted
// list of the 16 smallest (bits(dist2), j), of which the first k are the row.  No search structure.  A call the device would refuse for its
// query, rule or hit_stride changes nothing.
void gs4d_host_nearest_neighbours(size_t n, const float* rec, const gs4d_nearest_query* q, const gs4d_record_stat* source, const gs4d_keep_rule* rule,
                                  void* hits, size_t hit_stride, gs4d_record_stat* stats) {
    namespace nb = gs4d_neighbour;
    namespace nn = gs4d_nearest;
    if (!q || !nn::query_ok(*q) || !nn::stride_ok(hit_stride, q->k) || n >= 0xFFFFFFFFull || (source && !rule)) return;
    if (source && !rule_ok(rule)) return;
    const bool self = (q->flags & (uint32_t)GS4D_NN_INCLUDE_SELF) != 0u;
    const uint32_t skips = q->flags & (uint32_t)(GS4D_NN_SKIP_HIDDEN | GS4D_NN_SKIP_DEAD);
    const float rr = q->radius * q->radius;
    const Centres g(n, rec, q->t, skips, source, rule);
    const std::vector<float>& m = g.m;
    for (size_t i = 0; i < n; ++i) {
        uint64_t best[nn::K_MAX];
        for (uint64_t& b : best) b = nn::EMPTY;
        if (g.part[i])
            for (size_t j = 0; j < n; ++j)
                if (g.src[j] && (j != i || self) && nb::near(&m[3 * i], &m[3 * j], rr)) nn::insert(best, nn::order_key(nn::dist2(&m[3 * i], &m[3 * j]), (uint32_t)j));
        unsigned char* const row = (unsigned char*)hits + i * hit_stride;
        uint32_t f = 0;
        for (uint32_t p = 0; p < q->k; ++p) {
            const uint32_t slot[2] = { (uint32_t)best[p], (uint32_t)(best[p] >> 32) };      // {record, bits(dist2)}: a gs4d_neighbour_hit
            std::memcpy(row + 8 * p, slot, 8);
            if (best[p] != nn::EMPTY) f = p + 1u;
        }
        if (stats && f != 0u) add_fragments(stats[i], f, (uint32_t)(best[f - 1u] >> 32));
    }
}

int gs4d_host_measure_centre(const gs4d_measure* m, float centre3[3]) {
    centre3[0] = centre3[1] = centre3[2] = 0.0f;
    if (!m || m->count == 0u) return 0;
    const unsigned long long cell_sum[3] ={ m->cell_sum[0], m->cell_sum[1], m->cell_sum[2] };
    gs4d_transform::measure_centre(m->count, m->lo, m->hi, cell_sum, centre3);
    return 1;
}

// The definition of gs4d_transform_selected (gs4d.h), in place: the selection by the rule of gs4d_edit_colours; the pivot given, or
// gs4d_host_measure_centre of the measurement; a selected record is gs4d_transform::record_about of itself (csrc/transform_record.h).  A call the
// device would refuse for its xf changes nothing.
void gs4d_host_transform_selected(size_t n, float* rec, const gs4d_record_stat* stats, const gs4d_keep_rule* rule, const gs4d_selection_xf* xf,
                                  const gs4d_measure* measure) {
    if (!xf || xf->flags > (uint32_t)GS4D_XS_PIVOT_MEASURE) return;
    if (xf->flags == (uint32_t)GS4D_XS_PIVOT_MEASURE && !measure) return;
    if (stats && !rule) return;
    const bool pivot = xf->flags != 0u;
    float c[3] = { xf->pivot[0], xf->pivot[1], xf->pivot[2] };
    if (xf->flags == (uint32_t)GS4D_XS_PIVOT_MEASURE) gs4d_host_measure_centre(measure, c);
    for (size_t i = 0; i < n; ++i) {
        if (stats && !keeps(stats[i], rule)) continue;
        float* const p = rec + 24 * i;
        float out[24];
        gs4d_transform::record_about(xf->xf.l, xf->xf.o, pivot, c, p, out);
        std::memcpy(p, out, sizeof out);
    }
}

// "Frame selection" (gs4d.h): the bounding sphere of the box inside the narrower half-angle of gs4d_host_perspective's frustum — th is that
// function's own float tangent, aspect its own float quotient — seen along `orientation`.  In double.
void gs4d_host_frame_box(const float lo[3], const float hi[3], const float orientation[3], float fov_deg, int width, int height, float eye3[3]) {
    const float fovy = fov_deg * 0.01745329251994329576923690768489f;
    const double th = std::tan(fovy / 2.0f), aspect = (float)width / (float)height;
    const double half = std::atan(std::min(th, aspect * th));
    double c[3], r2 = 0.0, o2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        c[a] = 0.5 * ((double)lo[a] + (double)hi[a]);
        const double h = 0.5 * ((double)hi[a] - (double)lo[a]);
        r2 += h * h; o2 += (double)orientation[a] * (double)orientation[a];
    }
    double radius = std::sqrt(r2);
    if (!(radius > 0.0) || !std::isfinite(radius)) radius = 1.0;
    const double back = radius / std::sin(half) / std::sqrt(o2);
    for (int a = 0; a < 3; ++a) eye3[a] = (float)(c[a] - (double)orientation[a] * back);
}

void gs4d_host_affine4(const float q_wxyz[4], float scale, const float translate[3], const float velocity[3], float time_scale, float time_offset,
                       gs4d_affine4* out) {
    const M3 R = gs4d_build::rot_of({ q_wxyz[0], q_wxyz[1], q_wxyz[2], q_wxyz[3] });
    for (int c = 0; c < 3; ++c) {
        for (int r = 0; r < 3; ++r) out->l[4 * c + r] = scale * R.a[3 * c + r];
        out->l[4 * c + 3] = 0.0f;                              // the time row
        out->l[12 + c] = velocity[c];
        out->o[c] = translate[c];
    }
    out->l[15] = time_scale;
    out->o[3] = time_offset;
}

// ---- scene generators: the loops of LinearMotion::init (Scenes.h:258-279) and NonLinearMotion::init
//      (Scenes.h:517-545) with GetModelExtrema (:75-91) and GetColor (:58-68; Utils.cpp lerp/mapf, note mapf ignores `a` in the
//      numerator, Utils.cpp:130-133).  Pinned by the CRCs of the reference-generated SSBOs in tests/golden/manifest.json. ----
} // extern "C"

namespace {

inline float fminu(float a, float b) { return a < b ? a : b; }          // Utils::minf
inline float fmaxu(float a, float b) { return a > b ? a : b; }          // Utils::maxf
inline float lerpu(float a, float b, float t) { return a + ((b - a) * t); }
inline float mapfu(float x, float a, float b, float c, float d) { return c + ((x / (b - a)) * (d - c)); }
inline float clamp01(float x) { const float lo = (x < 0.0f) ? 0.0f : x; return (1.0f < lo) ? 1.0f : lo; }     // glm::clamp = min(max(x,0),1)

struct Extrema { float mn[3], mx[3]; };
Extrema extrema(const float* v6, size_t n) {
    Extrema e; for (int k = 0; k < 3; ++k) { e.mx[k] = -INFINITY; e.mn[k] = INFINITY; }
    for (size_t i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) { const float p = v6[6 * i + k]; e.mx[k] = fmaxu(p, e.mx[k]); e.mn[k] = fminu(p, e.mn[k]); }
    return e;
}
void get_color(const float pos[3], const Extrema& e, const float nrm[3], float out[4], float mina = 0.65f, float maxa = 1.0f, float lower = 0.0f) {
    const float t0 = 0.0f * nrm[0], t1 = -1.0f * nrm[1], t2 = 0.0f * nrm[2];
    const float d = (t0 + t1) + t2;                                       // glm::dot({0,-1,0}, normal)
    const float max_bright = mapfu(-d, -1.0f, 1.0f, mina, maxa);
    for (int k = 0; k < 3; ++k) out[k] = clamp01(lerpu(lower, max_bright, ((pos[k] - e.mn[k]) / (e.mx[k] - e.mn[k]))));
    out[3] = clamp01(1.0f);
}
// vec3(glm::rotate(vec4(v, 0), angle, vec3(0,1,0)))  (gtx/rotate_vector.inl:66-74 -> gtx/transform -> ext/matrix_transform.inl:18-46)
void rotate_about_y(const float v3[3], float angle, float out[3]) {
    const float c = std::cos(angle), s = std::sin(angle);
    const float inv = 1.0f / std::sqrt((0.0f * 0.0f + 1.0f * 1.0f) + 0.0f * 0.0f);
    const float ax[3] = { 0.0f * inv, 1.0f * inv, 0.0f * inv };
    const float tmp[3] = { (1.0f - c) * ax[0], (1.0f - c) * ax[1], (1.0f - c) * ax[2] };
    float Rm[3][3];
    Rm[0][0] = c + tmp[0] * ax[0];          Rm[0][1] = tmp[0] * ax[1] + s * ax[2]; Rm[0][2] = tmp[0] * ax[2] - s * ax[1];
    Rm[1][0] = tmp[1] * ax[0] - s * ax[2];  Rm[1][1] = c + tmp[1] * ax[1];         Rm[1][2] = tmp[1] * ax[2] + s * ax[0];
    Rm[2][0] = tmp[2] * ax[0] + s * ax[1];  Rm[2][1] = tmp[2] * ax[1] - s * ax[0]; Rm[2][2] = c + tmp[2] * ax[2];
    // Result[c] = I[0]*R[c][0] + I[1]*R[c][1] + I[2]*R[c][2]; Result[3] = I[3]
    float M[4][4];
    for (int cc = 0; cc < 3; ++cc) for (int r = 0; r < 4; ++r) {
        const float i0 = r == 0 ? 1.0f : 0.0f, i1 = r == 1 ? 1.0f : 0.0f, i2 = r == 2 ? 1.0f : 0.0f;
        M[cc][r] = (i0 * Rm[cc][0] + i1 * Rm[cc][1]) + i2 * Rm[cc][2];
    }
    for (int r = 0; r < 4; ++r) M[3][r] = r == 3 ? 1.0f : 0.0f;
    const float v[4] = { v3[0], v3[1], v3[2], 0.0f };
    for (int r = 0; r < 3; ++r) out[r] = (M[0][r] * v[0] + M[1][r] * v[1]) + (M[2][r] * v[2] + M[3][r] * v[3]);     // mat4*vec4: (Mul0+Mul1)+(Mul2+Mul3)
}
void rotate_forward_about_y(float angle, float out[3]) { const float fwd[3] = { 1.0f, 0.0f, 0.0f }; rotate_about_y(fwd, angle, out); }

constexpr float RAD = 0.01745329251994329576923690768489f;      // glm::radians

// One record from (position, time, facing normal, velocity, colour inputs): the tail every scene loop shares
// (Splat4D ctor Splat.h:132-159; quatLookAt + normalize; GetColor Scenes.h:58-68)
void make_record(const float pos[3], float t, const float face_normal[3], const float splat_scale[3], float lifetime, float fade, const float vel[3],
                 const float col_pos[3], const Extrema& e, const float col_normal[3], float* rec) {
    const float up[3] = { 0.0f, 1.0f, 0.0f };
    rec[0] = pos[0]; rec[1] = pos[1]; rec[2] = pos[2]; rec[3] = t;
    get_color(col_pos, e, col_normal, rec + 4);
    float q[4]; gs4d_host_quat_look_at(face_normal, up, q);
    gs4d_host_splat4d_cov(q, splat_scale, lifetime, fade, vel, rec + 8);
}

} // namespace

extern "C" {

void gs4d_host_scene_linear(size_t nverts, const float* verts6, int steps, float time_multiplier, float object_scale, const float splat_scale[3],
                            float lifetime, float fade, float speed, float* records24) {
    const Extrema e = extrema(verts6, nverts);
    const float up[3] = { 0.0f, 1.0f, 0.0f };
    size_t o = 0;
    for (int dt = 0; dt < steps; ++dt) for (size_t i = 0; i < nverts; ++i, ++o) {
        const float* pos = verts6 + 6 * i; const float* nrm = pos + 3;
        const float off = float(dt * time_multiplier);                      // dir * float(dt * m_lin_time_multiplyer), dir = (1,0,0)
        float* rec = records24 + 24 * o;
        rec[0] = (object_scale * pos[0]) + 1.0f * off; rec[1] = (object_scale * pos[1]) + 0.0f * off; rec[2] = (object_scale * pos[2]) + 0.0f * off; rec[3] = float(dt);
        get_color(pos, e, nrm, rec + 4);
        float q[4]; gs4d_host_quat_look_at(nrm, up, q);
        const float ninv = 1.0f / std::sqrt((1.0f * 1.0f + 0.0f * 0.0f) + 0.0f * 0.0f);   // glm::normalize(dir)
        const float dir[3] = { (1.0f * ninv) * speed, (0.0f * ninv) * speed, (0.0f * ninv) * speed };
        gs4d_host_splat4d_cov(q, splat_scale, lifetime, fade, dir, rec + 8);
    }
}

void gs4d_host_scene_nonlinear(size_t nverts, const float* verts6, int steps, float angle_multiplier, float radius, float object_scale,
                               const float splat_scale[3], float lifetime, float fade, float speed, size_t max_records, float* records24) {
    const Extrema e = extrema(verts6, nverts);
    const float up[3] = { 0.0f, 1.0f, 0.0f };
    size_t o = 0;
    for (int dt = 0; dt < steps && o < max_records; ++dt) {
        float cur[3], nxt[3];
        rotate_forward_about_y(float(dt * angle_multiplier) * RAD, cur);
        rotate_forward_about_y(float((dt + 1) * angle_multiplier) * RAD, nxt);
        for (size_t i = 0; i < nverts && o < max_records; ++i, ++o) {
            const float* pos = verts6 + 6 * i; const float* nrm = pos + 3;
            float* rec = records24 + 24 * o;
            for (int k = 0; k < 3; ++k) rec[k] = (object_scale * pos[k]) + (cur[k] * radius);
            rec[3] = float(dt);
            get_color(pos, e, nrm, rec + 4);
            float q[4]; gs4d_host_quat_look_at(nrm, up, q);
            const float dir[3] = { (nxt[0] - cur[0]) * speed, (nxt[1] - cur[1]) * speed, (nxt[2] - cur[2]) * speed };
            gs4d_host_splat4d_cov(q, splat_scale, lifetime, fade, dir, rec + 8);
        }
    }
}

// RotationMotion::init (Scenes.h:775-803): every vertex and its normal turn about the Y axis, 'angle_multiplier' degrees per time step.
void gs4d_host_scene_rotation(size_t nverts, const float* verts6, int steps, float angle_multiplier, float object_scale, const float splat_scale[3],
                              float lifetime, float fade, float speed, size_t max_records, float* records24) {
    const Extrema e = extrema(verts6, nverts);
    size_t o = 0;
    for (int dt = 0; dt < steps && o < max_records; ++dt) {
        const float a0 = float(dt * angle_multiplier) * RAD, a1 = float((dt + 1) * angle_multiplier) * RAD;
        for (size_t i = 0; i < nverts && o < max_records; ++i, ++o) {
            const float* pos = verts6 + 6 * i; const float* nrm = pos + 3;
            float cur[3], nxt[3], nr[3];
            rotate_about_y(pos, a0, cur); rotate_about_y(pos, a1, nxt); rotate_about_y(nrm, a0, nr);
            const float p[3] = { object_scale * cur[0], object_scale * cur[1], object_scale * cur[2] };
            const float vel[3] = { (nxt[0] - cur[0]) * speed, (nxt[1] - cur[1]) * speed, (nxt[2] - cur[2]) * speed };
            make_record(p, float(dt), nr, splat_scale, lifetime, fade, vel, pos, e, nrm, records24 + 24 * o);
        }
    }
}

// CombinedMotion::init (Scenes.h:1035-1068): rotation about Y plus a sine-wave translation along X.
void gs4d_host_scene_combined(size_t nverts, const float* verts6, int steps, float angle_multiplier, float lin_multiplier, float amplitude, float frequency,
                              float object_scale, const float splat_scale[3], float lifetime, float fade, float speed, size_t max_records, float* records24) {
    const Extrema e = extrema(verts6, nverts);
    size_t o = 0;
    for (int dt = 0; dt < steps && o < max_records; ++dt) {
        const float a0 = float(dt * angle_multiplier) * RAD, a1 = float((dt + 1) * angle_multiplier) * RAD;
        const float w0[3] = { lin_multiplier * (frequency * float(dt)), lin_multiplier * (amplitude * sinf(frequency * float(dt))), lin_multiplier * 0.0f };
        const float w1[3] = { lin_multiplier * (frequency * float(dt + 1)), lin_multiplier * (amplitude * sinf(frequency * float(dt + 1))), lin_multiplier * 0.0f };
        for (size_t i = 0; i < nverts && o < max_records; ++i, ++o) {
            const float* pos = verts6 + 6 * i; const float* nrm = pos + 3;
            const float md[3] = { object_scale * pos[0], object_scale * pos[1], object_scale * pos[2] };
            float r0[3], r1[3], nr[3];
            rotate_about_y(md, a0, r0); rotate_about_y(md, a1, r1); rotate_about_y(nrm, a0, nr);
            const float p[3] = { r0[0] + w0[0], r0[1] + w0[1], r0[2] + w0[2] };
            const float pn[3] = { r1[0] + w1[0], r1[1] + w1[1], r1[2] + w1[2] };
            const float vel[3] = { (pn[0] - p[0]) * speed, (pn[1] - p[1]) * speed, (pn[2] - p[2]) * speed };
            make_record(p, float(dt), nr, splat_scale, lifetime, fade, vel, pos, e, nrm, records24 + 24 * o);
        }
    }
}

// BrokenMotion::init (Scenes.h:1965-1989): the object jumps back every 20 steps (y = fmod(1 + dt, 20)).
void gs4d_host_scene_broken(size_t nverts, const float* verts6, int steps, float object_scale, const float splat_scale[3],
                            float lifetime, float fade, float speed, size_t max_records, float* records24) {
    const Extrema e = extrema(verts6, nverts);
    size_t o = 0;
    for (int dt = 0; dt < steps && o < max_records; ++dt) {
        const float pd[3] = { 1.0f + dt, std::fmod((1.0f + dt), 20.0f), 0.0f };
        const float pn[3] = { 1.0f + (dt + 1.0f), std::fmod((1.0f + (dt + 1.0f)), 20.0f), 0.0f };
        const float vel[3] = { (pn[0] - pd[0]) * speed, (pn[1] - pd[1]) * speed, (pn[2] - pd[2]) * speed };
        for (size_t i = 0; i < nverts && o < max_records; ++i, ++o) {
            const float* pos = verts6 + 6 * i; const float* nrm = pos + 3;
            const float p[3] = { (object_scale * pos[0]) + pd[0], (object_scale * pos[1]) + pd[1], (object_scale * pos[2]) + pd[2] };
            make_record(p, float(dt), nrm, splat_scale, lifetime, fade, vel, pos, e, nrm, records24 + 24 * o);
        }
    }
}

// SquareMotion::init (Scenes.h:2216-2259): the object walks the sides of a square in the XZ plane, steps/4 steps per side.
void gs4d_host_scene_square(size_t nverts, const float* verts6, int steps, float square_size, float object_scale, const float splat_scale[3],
                            float lifetime, float fade, float speed, size_t max_records, float* records24) {
    const Extrema e = extrema(verts6, nverts);
    size_t o = 0;
    int side = 0;
    const int per_side = steps / 4;
    if (per_side <= 0) return;                               // the reference divides by zero here (Scenes.h:2219-2220)
    const float delta = square_size / float(per_side);
    float pd[3] = { square_size / 2.0f, 0.0f, square_size / 2.0f };
    float pn[3] = { square_size / 2.0f + (delta * -1.0f), 0.0f + (delta * 0.0f), square_size / 2.0f + (delta * 0.0f) };
    static const float DIRS[4][3] = { { -1.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, -1.0f }, { 1.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 1.0f } };
    for (int dt = 0; dt < steps && o < max_records; ++dt) {
        float dir[3] = { 0.0f, 0.0f, 0.0f };
        if (dt > 0 && dt % per_side == 0) side += 1;
        if (side >= 0 && side < 4) for (int k = 0; k < 3; ++k) dir[k] = DIRS[side][k];
        for (int k = 0; k < 3; ++k) pd[k] = pd[k] + (delta * dir[k]);
        int s2 = side;
        if ((dt + 1) > 0 && (dt + 1) % per_side == 0) s2 += 1;
        if (s2 >= 0 && s2 < 4) for (int k = 0; k < 3; ++k) dir[k] = DIRS[s2][k];       // s2 == 4 keeps the direction of `side`
        for (int k = 0; k < 3; ++k) pn[k] = pn[k] + (delta * dir[k]);
        const float vel[3] = { (pn[0] - pd[0]) * speed, (pn[1] - pd[1]) * speed, (pn[2] - pd[2]) * speed };
        for (size_t i = 0; i < nverts && o < max_records; ++i, ++o) {
            const float* pos = verts6 + 6 * i; const float* nrm = pos + 3;
            const float p[3] = { (object_scale * pos[0]) + pd[0], (object_scale * pos[1]) + pd[1], (object_scale * pos[2]) + pd[2] };
            make_record(p, float(dt), nrm, splat_scale, lifetime, fade, vel, pos, e, nrm, records24 + 24 * o);
        }
    }
}

// VData::parse (VDataParser.h:25-58): whitespace-separated std::stof tokens, 6 per vertex (position, normal).
// Returns the number of vertices in the file (which may exceed cap_vertices; only cap_vertices are written), or -1 if it cannot be opened.
long gs4d_host_parse_vdata(const char* path, float* verts6, size_t cap_vertices) {
    std::ifstream file(path);
    if (!file.is_open()) return -1;
    std::vector<float> vals; std::string word;
    while (file >> word) vals.push_back(std::stof(word));
    const size_t n = vals.size() / 6;
    for (size_t i = 0; i < n && i < cap_vertices; ++i) std::memcpy(verts6 + 6 * i, vals.data() + 6 * i, 24);
    return (long)n;
}

// VData::parse_splat_data (VDataParser.h:60-123) followed by the ObjectDisplay record loop (Scenes.h:2483-2491): whitespace-separated
// std::stof tokens, 23 per splat — position(3), colour(4), 4x4 covariance column by column(16) — become 96-byte records
// {object_scale * position, 0 | colour | covariance}.  Returns the number of splats in the file (which may exceed cap_records; only
// cap_records are written), or -1 if it cannot be opened.  A trailing partial splat is ignored (the reference reads past the end there).
long gs4d_host_parse_sd(const char* path, float object_scale, float* records24, size_t cap_records) {
    std::ifstream file(path);
    if (!file.is_open()) return -1;
    std::vector<float> vals; std::string word;
    while (file >> word) vals.push_back(std::stof(word));
    const size_t n = vals.size() / 23;
    for (size_t i = 0; i < n && i < cap_records; ++i) {
        const float* w = vals.data() + 23 * i;
        float* rec = records24 + 24 * i;
        rec[0] = object_scale * w[0]; rec[1] = object_scale * w[1]; rec[2] = object_scale * w[2]; rec[3] = 0.0f;
        std::memcpy(rec + 4, w + 3, 16);
        std::memcpy(rec + 8, w + 7, 64);
    }
    return (long)n;
}

// Presentation: the packed RGBA8 frame (gs4d_read_pixels_rgba8_device, bottom row first like the GL window
// framebuffer the reference presents, Application.cpp:89, 186) as a PNG file, top row first.  Self-contained: stored (uncompressed)
// deflate blocks, CRC-32 and Adler-32 computed here.  Returns 0, or -1 if the file cannot be written.
int gs4d_host_write_png(const char* path, const uint8_t* rgba8, int width, int height) {
    if (!path || !rgba8 || width <= 0 || height <= 0) return -1;
    static uint32_t table[256]; static bool have = false;
    if (!have) { for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1; table[i] = c; } have = true; }
    auto crc = [&](uint32_t c, const uint8_t* p, size_t n) { for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8); return c; };
    auto be32 = [](uint8_t* o, uint32_t v) { o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v; };
    FILE* f = fopen(path, "wb");
    if (!f) return -1;
    bool ok = true;
    auto chunk = [&](const char type[4], const std::vector<uint8_t>& data) {
        uint8_t hdr[8]; be32(hdr, (uint32_t)data.size()); std::memcpy(hdr + 4, type, 4);
        uint32_t c = crc(0xFFFFFFFFu, hdr + 4, 4); c = crc(c, data.data(), data.size()) ^ 0xFFFFFFFFu;
        uint8_t tail[4]; be32(tail, c);
        ok = ok && fwrite(hdr, 1, 8, f) == 8 && (data.empty() || fwrite(data.data(), 1, data.size(), f) == data.size()) && fwrite(tail, 1, 4, f) == 4;
    };
    static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
    ok = fwrite(sig, 1, 8, f) == 8;
    std::vector<uint8_t> ihdr(13); be32(ihdr.data(), (uint32_t)width); be32(ihdr.data() + 4, (uint32_t)height);
    ihdr[8] = 8; ihdr[9] = 6; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;            // 8 bits, RGBA, deflate, no filter method, no interlace
    chunk("IHDR", ihdr);
    // raw scanlines: filter byte 0 + row, top row first (the framebuffer's row 0 is the bottom row)
    const size_t stride = (size_t)width * 4, raw_n = (stride + 1) * (size_t)height;
    std::vector<uint8_t> raw(raw_n);
    for (int y = 0; y < height; ++y) { uint8_t* o = raw.data() + (stride + 1) * (size_t)y; o[0] = 0; std::memcpy(o + 1, rgba8 + stride * (size_t)(height - 1 - y), stride); }
    std::vector<uint8_t> z; z.reserve(raw_n + raw_n / 65535 * 5 + 16);
    z.push_back(0x78); z.push_back(0x01);
    for (size_t off = 0; off < raw_n;) {
        const size_t n = std::min<size_t>(65535, raw_n - off);
        z.push_back(off + n == raw_n ? 1 : 0);
        z.push_back((uint8_t)(n & 255)); z.push_back((uint8_t)(n >> 8)); z.push_back((uint8_t)(~n & 255)); z.push_back((uint8_t)((~n >> 8) & 255));
        z.insert(z.end(), raw.begin() + off, raw.begin() + off + n);
        off += n;
    }
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < raw_n; ++i) { a = (a + raw[i]) % 65521u; b = (b + a) % 65521u; }
    uint8_t ad[4]; be32(ad, (b << 16) | a); z.insert(z.end(), ad, ad + 4);
    chunk("IDAT", z);
    chunk("IEND", {});
    ok = (fclose(f) == 0) && ok;
    return ok ? 0 : -1;
}

} // extern "C"

