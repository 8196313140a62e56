// depth_key.h — the depth key of one record, as plain C++ inline functions: the one text of the two key expressions.  k_keygen (csrc/sort.hip)
// writes it and blend_key_4d (csrc/preprocess.hip) derives a fused draw's blend order from it, so the two must give the same bits, or a fused draw
// blends in another order than the index it leaves behind.  float32, every product and every sum rounded on its own in the order the parentheses
// give (build without contraction), correctly rounded division and square root.  gs4d_host_key_bounds (host/gs4d_host.cpp) bounds ref_inv_euclid by
// the monotonicity of exactly these operations.
// p = (x, y, z, mu_t) and v = sig[3] = (velocity, Sigma44) of the record, t the time of the draw.
#ifndef GS4D_DEPTH_KEY_H
#define GS4D_DEPTH_KEY_H
#include <math.h>
#include "hd.h"

namespace gs4d_key {

// GS4D_KEY_REF_INV_EUCLID: the reference's key, 1 / the distance of the moved centre from the camera
GS4D_HD inline float ref_inv_euclid(float px, float py, float pz, float mu_t, float vx, float vy, float vz, float t, float camx, float camy, float camz) {
    float ct = t - mu_t;                                           // Scenes.h:30
    float x = px + vx * ct;                                        // :31-33  (sig[3].xyz, NOT divided by Sigma44)
    float y = py + vy * ct;
    float z = pz + vz * ct;
    float dx = x - camx, dy = y - camy, dz = z - camz;             // :317
    return 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);              // :318
}

// GS4D_KEY_VIEW_Z: 1 / the view-space depth of the shader's conditioned mean (Splat4DVertexShaderInstanced.GLSL:86); vr = row 2 of the view matrix
GS4D_HD inline float view_z(float px, float py, float pz, float mu_t, float vx, float vy, float vz, float s44, float t, float vr0, float vr1, float vr2, float vr3) {
    float k = (1.0f / s44) * (t - mu_t);
    float x = px + k * vx, y = py + k * vy, z = pz + k * vz;
    float zv = ((vr0 * x + vr1 * y) + vr2 * z) + vr3;
    return 1.0f / fmaxf(-zv, 1e-20f);
}

} // namespace gs4d_key
#endif
