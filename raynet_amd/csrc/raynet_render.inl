// raynet_render.inl -- a surface mesh seen from cameras: per pixel the face the ray hits first,
// its depth, where in the face (the Moeller-Trumbore u, v) and the vertices' colours and normals
// interpolated there (the definition is in include/raynet_hip.h at
// rn_mesh_render).  Included at the end of raynet_hip.hip, behind raynet_mesh.inl, whose BVH,
// leaf test and traversal it uses unchanged.
//
//   k_mesh_render   one lane per pixel, all views in one launch.  The ray and the depth are
//                   k_mesh_depthmap's, the first hit mesh_first_hit's.  The traversal carries no
//                   barycentrics: the winner's are formed afterwards, once, from faces[tri] and its
//                   three vertices with mesh_test_leaf's operations in its order -- the same inputs
//                   (k_mesh_leaves forms e1 and e2 the same way from the same fp32 vertices) and the
//                   same operations give the same bits, and the traversal keeps its registers.
//                   The attributes are interpolated in fp64, every operation rounded on its own.
//
// TILED: a wavefront covers an 8 x 8 tile of one view (its rays stay together in the BVH); else 64
// pixels of a row.  The result does not depend on the mapping; RENDER_TILED, one constant, chooses
// it when the library is built.

#include "raynet_render_args.h"

namespace {

constexpr bool RENDER_TILED = true;     // (tools/render_bench.py --build_rows builds the other one)

struct RenderArgs {
    const MeshNode *nodes;
    const MeshLeaf *leaves;
    int64_t nv, nf;
    const float *vertices;
    const int32_t *faces;
    const float *colors, *normals;      // either may be null
    int32_t C, V, H, W;
    const float *cameras;
    int32_t *face;
    float *depth, *bary, *color, *normal;
};

// a = (Wb a0 + U a1) + Vb a2 in fp64
__device__ __forceinline__ double render_mix(double Wb, double U, double Vb, float a0, float a1,
                                             float a2) {
    return (Wb * (double)a0 + U * (double)a1) + Vb * (double)a2;
}

template <bool TILED>
__global__ __launch_bounds__(MESH_RAY_BLOCK) void k_mesh_render(RenderArgs a) {
    __shared__ uint32_t stack[MESH_STACK * MESH_RAY_BLOCK];
    static_assert(MESH_RAY_BLOCK % rn_render::TILE_PIXELS == 0 && rn_render::TILE_PIXELS == WAVE,
                  "a tile is a wavefront");
    const int64_t lane = blockIdx.x * (int64_t)MESH_RAY_BLOCK + threadIdx.x;
    const rn_render::Pixel px =
        TILED ? rn_render::pixel_of_tile(lane / rn_render::TILE_PIXELS,
                                         (int)(lane % rn_render::TILE_PIXELS), a.V, a.H, a.W)
              : rn_render::pixel_of_row(lane, a.V, a.H, a.W);
    if (px.view < 0) return;
    const float *P_pinv = a.cameras + (size_t)rn_render::CAMERA_FLOATS * px.view;
    const float *center = P_pinv + 12;
    // the ray and the depth: k_mesh_depthmap's
    const int u = px.column, v = px.row;
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
        r[k] = (double)P_pinv[3 * k] * (double)u + (double)P_pinv[3 * k + 1] * (double)v +
               (double)P_pinv[3 * k + 2];
    const float cx = center[0], cy = center[1], cz = center[2];
    const float dx = (float)(r[0] / r[3]), dy = (float)(r[1] / r[3]), dz = (float)(r[2] / r[3]);
    const MeshBest b = mesh_first_hit(cx, cy, cz, dx, dy, dz, a.nodes, a.leaves,
                                      stack + threadIdx.x);
    float depth = 0.f;
    if (b.tri >= 0) {
        const double ex = (double)b.hx - (double)cx, ey = (double)b.hy - (double)cy,
                     ez = (double)b.hz - (double)cz;
        depth = (float)sqrt(ex * ex + ey * ey + ez * ez);
    }
    const size_t at = rn_render::pixel_index(px, a.H, a.W);
    a.face[at] = b.tri;
    a.depth[at] = depth;

    // the winner's vertices, where `faces` names three
    int32_t i0 = -1, i1 = -1, i2 = -1;
    if (rn_render::face_in(b.tri, a.nf)) {
        i0 = a.faces[rn_render::xyz_index(b.tri, 0)];
        i1 = a.faces[rn_render::xyz_index(b.tri, 1)];
        i2 = a.faces[rn_render::xyz_index(b.tri, 2)];
    }
    const bool known = rn_render::face_in(b.tri, a.nf) && rn_render::vertex_in(i0, a.nv) &&
                       rn_render::vertex_in(i1, a.nv) && rn_render::vertex_in(i2, a.nv);
    float bu = 0.f, bv = 0.f;
    if (known) {
        // mesh_first_hit's direction, then mesh_test_leaf's u and v
        float rx = dx - cx, ry = dy - cy, rz = dz - cz;
        const float norm = sqrtf(rx * rx + ry * ry + rz * rz);
        rx = rx / norm;
        ry = ry / norm;
        rz = rz / norm;
        const float *p0 = a.vertices + rn_render::xyz_index(i0, 0);
        const float *p1 = a.vertices + rn_render::xyz_index(i1, 0);
        const float *p2 = a.vertices + rn_render::xyz_index(i2, 0);
        const float p0x = p0[0], p0y = p0[1], p0z = p0[2];
        const float e1x = p1[0] - p0x, e1y = p1[1] - p0y, e1z = p1[2] - p0z;
        const float e2x = p2[0] - p0x, e2y = p2[1] - p0y, e2z = p2[2] - p0z;
        const float pvx = ry * e2z - rz * e2y, pvy = rz * e2x - rx * e2z, pvz = rx * e2y - ry * e2x;
        const float det = e1x * pvx + e1y * pvy + e1z * pvz;
        const float inv = 1.f / det;
        const float tx = cx - p0x, ty = cy - p0y, tz = cz - p0z;
        bu = (tx * pvx + ty * pvy + tz * pvz) * inv;
        const float qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
        bv = (rx * qx + ry * qy + rz * qz) * inv;
    }
    a.bary[2 * at] = bu;
    a.bary[2 * at + 1] = bv;
    const double U = (double)bu, Vb = (double)bv, Wb = (1.0 - U) - Vb;
    if (a.colors) {
        for (int c = 0; c < a.C; c++) {
            float out = 0.f;
            if (known)
                out = (float)render_mix(Wb, U, Vb, a.colors[(size_t)i0 * a.C + c],
                                        a.colors[(size_t)i1 * a.C + c],
                                        a.colors[(size_t)i2 * a.C + c]);
            a.color[at * a.C + c] = out;
        }
    }
    if (a.normals) {
        float out[3] = {0.f, 0.f, 0.f};
        if (known) {
            double n[3];
#pragma unroll
            for (int k = 0; k < 3; k++)
                n[k] = render_mix(Wb, U, Vb, a.normals[rn_render::xyz_index(i0, k)],
                                  a.normals[rn_render::xyz_index(i1, k)],
                                  a.normals[rn_render::xyz_index(i2, k)]);
            const double l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
            if (l2 > 0.0 && l2 < (double)INFINITY) {
                const double l = sqrt(l2);
#pragma unroll
                for (int k = 0; k < 3; k++) out[k] = (float)(n[k] / l);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) a.normal[rn_render::xyz_index(at, k)] = out[k];
    }
}

}  // namespace

extern "C" {

int rn_mesh_render(rn_ctx *ctx, const float *nodes, const float *leaves, int64_t nv,
                   const float *vertices, int64_t nf, const int32_t *faces, const float *colors,
                   int32_t C, const float *normals, int32_t V, const float *cameras, int32_t H,
                   int32_t W, int32_t *face, float *depth, float *bary, float *color, float *normal,
                   void *stream) {
    const rn_render::Verdict verdict =
        rn_render::render_args(ctx != nullptr, nodes, leaves, nv, vertices, nf, faces, colors, C,
                               normals, V, cameras, H, W, face, depth, bary, color, normal);
    if (verdict == rn_render::INVALID)
        return fail(ctx, RN_ERR_INVALID,
                    "rn_mesh_render: bad argument (nv %lld, nf %lld, C %d, V %d, H %d, W %d)",
                    (long long)nv, (long long)nf, (int)C, (int)V, (int)H, (int)W);
    if (verdict == rn_render::EMPTY) return RN_OK;
    const RenderArgs a{reinterpret_cast<const MeshNode *>(nodes),
                       reinterpret_cast<const MeshLeaf *>(leaves), nv, nf, vertices, faces, colors,
                       normals, C, V, H, W, cameras, face, depth, bary, color, normal};
    const int64_t lanes = RENDER_TILED ? rn_render::lanes_tiled(V, H, W) : rn_render::lanes_rows(V, H, W);
    hipLaunchKernelGGL(k_mesh_render<RENDER_TILED>,
                       dim3((unsigned)rn_render::blocks(lanes, MESH_RAY_BLOCK)),
                       dim3(MESH_RAY_BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
