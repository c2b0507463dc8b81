// raynet_mesh.inl -- ground truth from scene meshes: the first intersection of rays with a
// triangle mesh through a bounding volume hierarchy built on the GPU.  Included at the end of
// raynet_hip.hip.
//
//   k_mesh_keys       30-bit Morton code of every triangle's centroid, quantised in the
//                     mesh's box, as the 64-bit key `code << 32 | triangle index`
//   k_mesh_leaves     the leaves in key order: p0, e1 = p1 - p0, e2 = p2 - p0 (fp32, the bits
//                     raynet/utils/fast_utils.pyx:80-81 computes) and the triangle's index
//   k_mesh_hierarchy  the Karras (2012) radix tree over the sorted keys, one triangle per leaf
//   k_mesh_boxes      the two child boxes of every internal node: min / max over the child's
//                     contiguous leaf range (one wavefront per node) -- exact, one launch and
//                     no hand-off between workgroups
//   k_mesh_depth      the tree's depth (the traversal stack's guard)
//   k_mesh_raycast    first intersection of explicit rays (one lane per ray)
//   k_mesh_depthmap   first intersection of every pixel's ray -> distance map
//   k_mesh_closest    the nearest point of the mesh for every query point (float64 leaf test)
//   k_mesh_areas      triangle areas in float64
//   k_mesh_sample     stratified, area-weighted points of the surface from a counter hash
//
// The intersection test restates fast_ray_triangles_intersection (fast_utils.pyx:47-117,
// Moeller-Trumbore) operation for operation in fp32 with correctly rounded division and
// square root (the library builds with -ffp-contract=off and HIP's correctly rounded fp32
// division / sqrt); the winner is the hit with the smallest fp32 key
// ((hx-ox)^2 + (hy-oy)^2) + (hz-oz)^2, the lower triangle index on equal keys
// (training_utils.py:194-220: argmin over candidates in index order).  Only hits with t >= 0
// count; every hit counts (the reference keeps the first 100).  DESIGN.md section 14.

namespace {

constexpr int MESH_STACK = 64;            // traversal stack entries per lane: depth <= 63
constexpr int MESH_RAY_BLOCK = 128;       // k_mesh_raycast / k_mesh_depthmap workgroup size
constexpr uint32_t MESH_LEAF = 0x80000000u;
// relative widening of the slab test (pruning only): a node is visited unless it is further
// than this fraction of the scene's scale away from the ray -- rounding in the intersection
// test moves a hit by a few ulps of these magnitudes, far less than this margin
constexpr float MESH_MARGIN = 1e-4f;

// internal node: the boxes of both children; child references in a_lo.w / b_lo.w (bits):
// an internal node's index, or MESH_LEAF | leaf index
struct MeshNode {
    float4 a_lo, a_hi, b_lo, b_hi;
};
// leaf in key order: p0.w holds the original triangle index (bits)
struct MeshLeaf {
    float4 p0, e1, e2;
};

__device__ __forceinline__ uint32_t morton_spread10(uint32_t x) {
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__device__ __forceinline__ uint32_t morton_cell(float c, float lo, float hi) {
    const float ext = hi - lo;
    if (!(ext > 0.f)) return 0u;
    const float q = fminf(fmaxf((c - lo) / ext * 1024.f, 0.f), 1023.f);    // NaN -> 0
    return (uint32_t)q;
}

// keys[i] = morton(centroid of triangle i) << 32 | i; box = mesh lo xyz, hi xyz
__global__ __launch_bounds__(BLOCK) void k_mesh_keys(int n, const float *__restrict__ tris,
                                                     const float *__restrict__ box,
                                                     unsigned long long *__restrict__ keys) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float *t = tris + (size_t)9 * i;
    uint32_t code = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float c = (t[k] + t[3 + k] + t[6 + k]) / 3.f;
        code |= morton_spread10(morton_cell(c, box[k], box[3 + k])) << (2 - k);
    }
    keys[i] = ((unsigned long long)code << 32) | (unsigned long long)(uint32_t)i;
}

// leaves and their boxes (lo, hi) in key order
__global__ __launch_bounds__(BLOCK) void k_mesh_leaves(int n, const float *__restrict__ tris,
                                                       const unsigned long long *__restrict__ keys,
                                                       MeshLeaf *__restrict__ leaves,
                                                       float4 *__restrict__ leaf_box) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t idx = (uint32_t)(keys[i] & 0xffffffffull);
    const float *t = tris + (size_t)9 * idx;
    const float p0x = t[0], p0y = t[1], p0z = t[2];
    const float p1x = t[3], p1y = t[4], p1z = t[5];
    const float p2x = t[6], p2y = t[7], p2z = t[8];
    MeshLeaf L;
    L.p0 = make_float4(p0x, p0y, p0z, __uint_as_float(idx));
    L.e1 = make_float4(p1x - p0x, p1y - p0y, p1z - p0z, 0.f);
    L.e2 = make_float4(p2x - p0x, p2y - p0y, p2z - p0z, 0.f);
    leaves[i] = L;
    leaf_box[2 * (size_t)i] = make_float4(fminf(fminf(p0x, p1x), p2x), fminf(fminf(p0y, p1y), p2y),
                                          fminf(fminf(p0z, p1z), p2z), 0.f);
    leaf_box[2 * (size_t)i + 1] = make_float4(fmaxf(fmaxf(p0x, p1x), p2x),
                                              fmaxf(fmaxf(p0y, p1y), p2y),
                                              fmaxf(fmaxf(p0z, p1z), p2z), 0.f);
}

// common-prefix length of keys a and b (-1 outside the list); keys are unique
__device__ __forceinline__ int mesh_delta(const unsigned long long *keys, int n, int a, int b) {
    if (b < 0 || b >= n) return -1;
    return __clzll(keys[a] ^ keys[b]);
}

// Karras (2012), Figure 4: internal node i covers leaves [first, last], split between `split`
// and split + 1.  ranges[i] = (first, last, split); parent[] over the node ids 0 .. n_int - 1
// (internal) and n_int + k (leaf k).  One leaf: one internal node over [0, 0].
__global__ __launch_bounds__(BLOCK) void k_mesh_hierarchy(int n, int n_int,
                                                          const unsigned long long *__restrict__ keys,
                                                          int4 *__restrict__ ranges,
                                                          int *__restrict__ parent) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_int) return;
    if (i == 0) parent[0] = -1;
    if (n == 1) {
        ranges[0] = make_int4(0, 0, 0, 0);
        parent[n_int] = 0;
        return;
    }
    const int d = mesh_delta(keys, n, i, i + 1) > mesh_delta(keys, n, i, i - 1) ? 1 : -1;
    const int dmin = mesh_delta(keys, n, i, i - d);
    long long lmax = 2;
    while (mesh_delta(keys, n, i, (int)(i + lmax * d)) > dmin) lmax *= 2;
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (mesh_delta(keys, n, i, (int)(i + (l + t) * d)) > dmin) l += t;
    const int j = (int)(i + l * d);
    const int dnode = mesh_delta(keys, n, i, j);
    long long s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (mesh_delta(keys, n, i, (int)(i + (s + t) * d)) > dnode) s += t;
    } while (t > 1);
    const int split = (int)(i + s * d + (d < 0 ? -1 : 0));
    const int first = min(i, j), last = max(i, j);
    ranges[i] = make_int4(first, last, split, 0);
    parent[first == split ? n_int + split : split] = i;
    parent[last == split + 1 ? n_int + split + 1 : split + 1] = i;
}

__device__ __forceinline__ void mesh_box_range(const float4 *__restrict__ leaf_box, int first,
                                               int last, int lane, float4 &lo, float4 &hi) {
    lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
    hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    for (int k = first + lane; k <= last; k += WAVE) {
        const float4 a = leaf_box[2 * (size_t)k], b = leaf_box[2 * (size_t)k + 1];
        lo.x = fminf(lo.x, a.x); lo.y = fminf(lo.y, a.y); lo.z = fminf(lo.z, a.z);
        hi.x = fmaxf(hi.x, b.x); hi.y = fmaxf(hi.y, b.y); hi.z = fmaxf(hi.z, b.z);
    }
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m /= 2) {
        lo.x = fminf(lo.x, __shfl_xor(lo.x, m)); lo.y = fminf(lo.y, __shfl_xor(lo.y, m));
        lo.z = fminf(lo.z, __shfl_xor(lo.z, m));
        hi.x = fmaxf(hi.x, __shfl_xor(hi.x, m)); hi.y = fmaxf(hi.y, __shfl_xor(hi.y, m));
        hi.z = fmaxf(hi.z, __shfl_xor(hi.z, m));
    }
}

// one wavefront per internal node: both children's boxes over their leaf ranges
__global__ __launch_bounds__(BLOCK) void k_mesh_boxes(int n_int, const int4 *__restrict__ ranges,
                                                      const float4 *__restrict__ leaf_box,
                                                      MeshNode *__restrict__ nodes) {
    const int w = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (w >= n_int) return;                       // uniform per wavefront
    const int4 r = ranges[w];
    int a0 = r.x, a1 = r.z, b0 = r.z + 1, b1 = r.y;
    if (r.x == r.y) b0 = b1 = r.x;                // one leaf: both children are leaf 0
    MeshNode nd;
    mesh_box_range(leaf_box, a0, a1, lane, nd.a_lo, nd.a_hi);
    mesh_box_range(leaf_box, b0, b1, lane, nd.b_lo, nd.b_hi);
    nd.a_lo.w = __uint_as_float(a0 == a1 ? (MESH_LEAF | (uint32_t)a0) : (uint32_t)r.z);
    nd.b_lo.w = __uint_as_float(b0 == b1 ? (MESH_LEAF | (uint32_t)b0) : (uint32_t)(r.z + 1));
    if (lane == 0) nodes[w] = nd;
}

// depth of the deepest leaf (edges from the root) -> atomicMax into *depth
__global__ __launch_bounds__(BLOCK) void k_mesh_depth(int n, int n_int, const int *__restrict__ parent,
                                                      int *depth) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    int d = 0;
    if (k < n) {
        int id = n_int + k;
        // a well-formed tree reaches the root within 63 steps; the bound only ends the walk of
        // a malformed one, whose depth then fails the guard
        while (id > 0 && d <= 4 * MESH_STACK) {
            id = parent[id];
            d++;
        }
    }
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m /= 2) d = max(d, __shfl_xor(d, m));
    if (threadIdx.x % WAVE == 0) atomicMax(depth, d);
}

// one axis of the slab test: the ray's t interval inside [lo, hi]; a ray parallel to the axis
// (r == 0) is either inside the (widened) slab for every t or for none
__device__ __forceinline__ void mesh_axis(float lo, float hi, float o, float r, float inv, float m,
                                          float &tn, float &tf, bool &in) {
    if (r != 0.f) {
        const float a = (lo - o) * inv, b = (hi - o) * inv;
        tn = fmaxf(tn, fminf(a, b));
        tf = fminf(tf, fmaxf(a, b));
    } else if (o < lo - m || o > hi + m) {
        in = false;
    }
}

// slab test of a node box against the ray, the interval widened by `m` (plus a relative share
// of its far end) on both sides; true if the box may hold a hit with 0 <= t <= lim
__device__ __forceinline__ bool mesh_slab(float4 lo, float4 hi, float ox, float oy, float oz,
                                          float rx, float ry, float rz, float ix, float iy,
                                          float iz, float m, float lim, float &tnear) {
    float tn = -INFINITY, tf = INFINITY;
    bool in = true;
    mesh_axis(lo.x, hi.x, ox, rx, ix, m, tn, tf, in);
    mesh_axis(lo.y, hi.y, oy, ry, iy, m, tn, tf, in);
    mesh_axis(lo.z, hi.z, oz, rz, iz, m, tn, tf, in);
    const float mm = m + MESH_MARGIN * fabsf(tf);
    tnear = tn;
    return in && tn - mm <= tf + mm && tf + mm >= 0.f && tn - mm <= lim;
}

struct MeshBest {
    float key;
    int tri;          // original triangle index, -1: no hit
    float hx, hy, hz;
};

// fast_ray_triangles_intersection's body for one triangle, then the argmin rule
__device__ __forceinline__ void mesh_test_leaf(const MeshLeaf &L, float ox, float oy, float oz,
                                               float rx, float ry, float rz, MeshBest &b) {
    const float e1x = L.e1.x, e1y = L.e1.y, e1z = L.e1.z;
    const float e2x = L.e2.x, e2y = L.e2.y, e2z = L.e2.z;
    const float px = ry * e2z - rz * e2y, py = rz * e2x - rx * e2z, pz = rx * e2y - ry * e2x;
    const float det = e1x * px + e1y * py + e1z * pz;
    if (-1e-6f < det && det < 1e-6f) return;
    const float inv = 1.f / det;
    const float tx = ox - L.p0.x, ty = oy - L.p0.y, tz = oz - L.p0.z;
    const float u = (tx * px + ty * py + tz * pz) * inv;
    if (u < 0.f || u > 1.f) return;
    const float qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
    const float v = (rx * qx + ry * qy + rz * qz) * inv;
    if (v < 0.f || u + v > 1.f) return;
    const float t = (e2x * qx + e2y * qy + e2z * qz) * inv;
    if (!(t >= 0.f)) return;
    const float hx = ox + t * rx, hy = oy + t * ry, hz = oz + t * rz;
    const float dx = hx - ox, dy = hy - oy, dz = hz - oz;
    const float key = dx * dx + dy * dy + dz * dz;
    const int tri = (int)__float_as_uint(L.p0.w);
    if (key < b.key || (key == b.key && tri < b.tri)) {
        b.key = key;
        b.tri = tri;
        b.hx = hx;
        b.hy = hy;
        b.hz = hz;
    }
}

// first hit of the ray from o towards dst; `stack` is this lane's first LDS stack entry
// (entries MESH_RAY_BLOCK apart).  Nearer child first, the other one pushed.
__device__ __forceinline__ MeshBest mesh_first_hit(float ox, float oy, float oz, float dx, float dy,
                                                   float dz, const MeshNode *__restrict__ nodes,
                                                   const MeshLeaf *__restrict__ leaves,
                                                   uint32_t *stack) {
    // ray = (dst - o) / sqrt(|dst - o|^2), fast_utils.pyx:56-63
    float rx = dx - ox, ry = dy - oy, rz = dz - oz;
    const float norm = sqrtf(rx * rx + ry * ry + rz * rz);
    rx = rx / norm;
    ry = ry / norm;
    rz = rz / norm;
    // slab test inputs (pruning only, no exactness needed; unused where a component is 0)
    const float ix = 1.f / rx, iy = 1.f / ry, iz = 1.f / rz;
    const MeshNode root = nodes[0];
    const float scale = fmaxf(fmaxf(fmaxf(fabsf(root.a_lo.x), fabsf(root.a_lo.y)), fabsf(root.a_lo.z)),
                              fmaxf(fmaxf(fabsf(root.a_hi.x), fabsf(root.a_hi.y)), fabsf(root.a_hi.z)));
    const float scale_b = fmaxf(fmaxf(fmaxf(fabsf(root.b_lo.x), fabsf(root.b_lo.y)), fabsf(root.b_lo.z)),
                                fmaxf(fmaxf(fabsf(root.b_hi.x), fabsf(root.b_hi.y)), fabsf(root.b_hi.z)));
    const float m = MESH_MARGIN * (fmaxf(scale, scale_b) +
                                   fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz)));
    MeshBest b;
    b.key = INFINITY;
    b.tri = -1;
    b.hx = b.hy = b.hz = 0.f;
    uint32_t node = 0;
    int sp = 0;
    while (true) {
        const MeshNode nd = nodes[node];
        const float lim = sqrtf(b.key) * (1.f + MESH_MARGIN) + m;
        float ta, tb;
        bool ha = mesh_slab(nd.a_lo, nd.a_hi, ox, oy, oz, rx, ry, rz, ix, iy, iz, m, lim, ta);
        bool hb = mesh_slab(nd.b_lo, nd.b_hi, ox, oy, oz, rx, ry, rz, ix, iy, iz, m, lim, tb);
        const uint32_t ca = __float_as_uint(nd.a_lo.w), cb = __float_as_uint(nd.b_lo.w);
        if (ha && (ca & MESH_LEAF)) {
            mesh_test_leaf(leaves[ca & ~MESH_LEAF], ox, oy, oz, rx, ry, rz, b);
            ha = false;
        }
        if (hb && (cb & MESH_LEAF)) {
            mesh_test_leaf(leaves[cb & ~MESH_LEAF], ox, oy, oz, rx, ry, rz, b);
            hb = false;
        }
        if (ha && hb) {
            const bool a_first = ta <= tb;
            stack[sp * MESH_RAY_BLOCK] = a_first ? cb : ca;
            sp++;
            node = a_first ? ca : cb;
        } else if (ha) {
            node = ca;
        } else if (hb) {
            node = cb;
        } else {
            if (sp == 0) break;
            sp--;
            node = stack[sp * MESH_RAY_BLOCK];
        }
    }
    return b;
}

// explicit rays: origins / destinations [n][3] f32 -> points [n][3] f32, tri [n] (-1: miss)
__global__ __launch_bounds__(MESH_RAY_BLOCK) void k_mesh_raycast(int n, const float *__restrict__ origins,
                                                                 const float *__restrict__ dests,
                                                                 const MeshNode *__restrict__ nodes,
                                                                 const MeshLeaf *__restrict__ leaves,
                                                                 float *__restrict__ points,
                                                                 int32_t *__restrict__ tri) {
    __shared__ uint32_t stack[MESH_STACK * MESH_RAY_BLOCK];
    const int i = blockIdx.x * MESH_RAY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t o = 3 * (size_t)i;
    const MeshBest b = mesh_first_hit(origins[o], origins[o + 1], origins[o + 2], dests[o],
                                      dests[o + 1], dests[o + 2], nodes, leaves,
                                      stack + threadIdx.x);
    points[o] = b.hx;
    points[o + 1] = b.hy;
    points[o + 2] = b.hz;
    tri[i] = b.tri;
}

// pixel i = u*H + v (k_depth_points' order): ray from the centre to project(P_pinv, (u, v, 1))
// formed in float64 from the fp32 P_pinv [4][3] and rounded once to fp32; depth [H][W] f32 =
// distance of the hit to the centre (float64, then rounded), 0 where the ray hits nothing
__global__ __launch_bounds__(MESH_RAY_BLOCK) void k_mesh_depthmap(int H, int W, const float *__restrict__ P_pinv,
                                                                  const float *__restrict__ center,
                                                                  const MeshNode *__restrict__ nodes,
                                                                  const MeshLeaf *__restrict__ leaves,
                                                                  float *__restrict__ depth) {
    __shared__ uint32_t stack[MESH_STACK * MESH_RAY_BLOCK];
    const int i = blockIdx.x * MESH_RAY_BLOCK + threadIdx.x;
    if (i >= H * W) return;
    const int u = i / H, v = i % H;
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
        r[k] = (double)P_pinv[3 * k] * (double)u + (double)P_pinv[3 * k + 1] * (double)v +
               (double)P_pinv[3 * k + 2];
    const float cx = center[0], cy = center[1], cz = center[2];
    const MeshBest b = mesh_first_hit(cx, cy, cz, (float)(r[0] / r[3]), (float)(r[1] / r[3]),
                                      (float)(r[2] / r[3]), nodes, leaves, stack + threadIdx.x);
    float out = 0.f;
    if (b.tri >= 0) {
        const double ex = (double)b.hx - (double)cx, ey = (double)b.hy - (double)cy,
                     ez = (double)b.hz - (double)cz;
        out = (float)sqrt(ex * ex + ey * ey + ez * ez);
    }
    depth[(size_t)v * W + u] = out;
}

// ---- nearest point on the mesh, areas, area-weighted surface samples -----------------------
// The surface is the set of the leaves' triangles: a = p0, b = p0 + e1, c = p0 + e2, the fp32
// leaf values widened to float64 (the triangles the ray cast intersects).

struct MeshNear {
    double d2;            // squared distance of the best triangle so far
    double cx, cy, cz;    // the point of it that attains d2
    int tri;              // its original index
};

// Closest point of one triangle to q in float64: the region classification of Ericson,
// Real-Time Collision Detection 5.1.5.  An edge's region counts only where the edge has a length
// (the quotient's denominator, its squared length, is > 0): with a == b every term of "edge ab"
// is zero and the unguarded rule would claim every point; a collapsed edge is left to the vertex
// regions and the other edges, so a triangle collapsed to a segment or a point is that segment
// or point, and nothing here can form 0 / 0.
__device__ __forceinline__ void mesh_closest_leaf(const MeshLeaf &L, double qx, double qy,
                                                  double qz, MeshNear &best) {
    const double ax = L.p0.x, ay = L.p0.y, az = L.p0.z;
    const double abx = L.e1.x, aby = L.e1.y, abz = L.e1.z;
    const double acx = L.e2.x, acy = L.e2.y, acz = L.e2.z;
    const double apx = qx - ax, apy = qy - ay, apz = qz - az;
    const double d1 = abx * apx + aby * apy + abz * apz;
    const double d2 = acx * apx + acy * apy + acz * apz;
    double v = 0., w = 0.;
    if (!(d1 <= 0. && d2 <= 0.)) {                                        // else: vertex a
        const double bpx = qx - (ax + abx), bpy = qy - (ay + aby), bpz = qz - (az + abz);
        const double d3 = abx * bpx + aby * bpy + abz * bpz;
        const double d4 = acx * bpx + acy * bpy + acz * bpz;
        const double vc = d1 * d4 - d3 * d2;
        if (d3 >= 0. && d4 <= d3) {                                       // vertex b
            v = 1.;
        } else if (vc <= 0. && d1 >= 0. && d3 <= 0. && d1 - d3 > 0.) {    // edge ab
            v = d1 / (d1 - d3);
        } else {
            const double cpx = qx - (ax + acx), cpy = qy - (ay + acy), cpz = qz - (az + acz);
            const double d5 = abx * cpx + aby * cpy + abz * cpz;
            const double d6 = acx * cpx + acy * cpy + acz * cpz;
            const double vb = d5 * d2 - d1 * d6;
            const double va = d3 * d6 - d5 * d4;
            if (d6 >= 0. && d5 <= d6) {                                   // vertex c
                w = 1.;
            } else if (vb <= 0. && d2 >= 0. && d6 <= 0. && d2 - d6 > 0.) {    // edge ac
                w = d2 / (d2 - d6);
            } else if (va <= 0. && d4 - d3 >= 0. && d5 - d6 >= 0. &&
                       (d4 - d3) + (d5 - d6) > 0.) {                      // edge bc
                w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
                v = 1. - w;
            } else {                                                      // the face
                const double den = va + vb + vc;
                if (den > 0.) {
                    v = fmin(fmax(vb / den, 0.), 1.);
                    w = fmin(fmax(vc / den, 0.), 1. - v);
                }
            }
        }
    }
    const double cx = (ax + v * abx) + w * acx, cy = (ay + v * aby) + w * acy,
                 cz = (az + v * abz) + w * acz;
    const double ex = qx - cx, ey = qy - cy, ez = qz - cz;
    const double dd = ex * ex + ey * ey + ez * ez;
    if (dd < best.d2) {
        best.d2 = dd;
        best.cx = cx;
        best.cy = cy;
        best.cz = cz;
        best.tri = (int)__float_as_uint(L.p0.w);
    }
}

// fp32 distance of (x, y, z) to a box, then made a lower bound of the float64 distance of the
// query to anything in the box: shrunk by MESH_MARGIN of itself and by `m` (pruning only)
__device__ __forceinline__ float mesh_box_lower(float4 lo, float4 hi, float x, float y, float z,
                                                float m) {
    const float dx = fmaxf(fmaxf(lo.x - x, x - hi.x), 0.f);
    const float dy = fmaxf(fmaxf(lo.y - y, y - hi.y), 0.f);
    const float dz = fmaxf(fmaxf(lo.z - z, z - hi.z), 0.f);
    return sqrtf(dx * dx + dy * dy + dz * dz) * (1.f - MESH_MARGIN) - m;
}

// an fp32 upper bound of the best distance so far
__device__ __forceinline__ float mesh_near_limit(const MeshNear &b) {
    return sqrtf((float)b.d2) * (1.f + MESH_MARGIN);
}

// One lane per query.  The children of a node are tested when the node is taken up -- a popped
// node is not tested again as a whole, its box is not stored in it: one fetch more for a
// node the search has meanwhile overtaken, and the stack stays one 32-bit word per entry.
__global__ __launch_bounds__(MESH_RAY_BLOCK) void k_mesh_closest(int n, const double *__restrict__ queries,
                                                                 const MeshNode *__restrict__ nodes,
                                                                 const MeshLeaf *__restrict__ leaves,
                                                                 double *__restrict__ dist,
                                                                 double *__restrict__ closest,
                                                                 int32_t *__restrict__ tri) {
    __shared__ uint32_t stack_all[MESH_STACK * MESH_RAY_BLOCK];
    const int i = blockIdx.x * MESH_RAY_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t *stack = stack_all + threadIdx.x;
    const size_t o = 3 * (size_t)i;
    const double qx = queries[o], qy = queries[o + 1], qz = queries[o + 2];
    const float fx = (float)qx, fy = (float)qy, fz = (float)qz;
    const MeshNode root = nodes[0];
    const float scale = fmaxf(fmaxf(fmaxf(fabsf(root.a_lo.x), fabsf(root.a_lo.y)), fabsf(root.a_lo.z)),
                              fmaxf(fmaxf(fabsf(root.a_hi.x), fabsf(root.a_hi.y)), fabsf(root.a_hi.z)));
    const float scale_b = fmaxf(fmaxf(fmaxf(fabsf(root.b_lo.x), fabsf(root.b_lo.y)), fabsf(root.b_lo.z)),
                                fmaxf(fmaxf(fabsf(root.b_hi.x), fabsf(root.b_hi.y)), fabsf(root.b_hi.z)));
    // the absolute margin: rounding q to fp32 moves it by 2^-24 |q|, a leaf's b and c lie
    // within 2^-23 of the scene's scale of the fp32 vertices the boxes hold
    const float m = MESH_MARGIN * (fmaxf(scale, scale_b) +
                                   fmaxf(fmaxf(fabsf(fx), fabsf(fy)), fabsf(fz)));
    MeshNear b;
    b.d2 = INFINITY;
    b.cx = b.cy = b.cz = 0.;
    b.tri = -1;
    uint32_t node = 0;
    int sp = 0;
    while (true) {
        const MeshNode nd = nodes[node];
        const float da = mesh_box_lower(nd.a_lo, nd.a_hi, fx, fy, fz, m);
        const float db = mesh_box_lower(nd.b_lo, nd.b_hi, fx, fy, fz, m);
        const uint32_t ca = __float_as_uint(nd.a_lo.w), cb = __float_as_uint(nd.b_lo.w);
        // (a child is skipped only where `lower > limit` holds: a NaN query skips nothing)
        bool ha = true, hb = true;
        if (ca & MESH_LEAF) {
            if (!(da > mesh_near_limit(b))) mesh_closest_leaf(leaves[ca & ~MESH_LEAF], qx, qy, qz, b);
            ha = false;
        }
        if (cb & MESH_LEAF) {
            if (!(db > mesh_near_limit(b))) mesh_closest_leaf(leaves[cb & ~MESH_LEAF], qx, qy, qz, b);
            hb = false;
        }
        const float lim = mesh_near_limit(b);
        ha = ha && !(da > lim);
        hb = hb && !(db > lim);
        if (ha && hb) {
            const bool a_first = da <= db;
            stack[sp * MESH_RAY_BLOCK] = a_first ? cb : ca;
            sp++;
            node = a_first ? ca : cb;
        } else if (ha) {
            node = ca;
        } else if (hb) {
            node = cb;
        } else {
            if (sp == 0) break;
            sp--;
            node = stack[sp * MESH_RAY_BLOCK];
        }
    }
    dist[i] = sqrt(b.d2);
    if (closest) {
        closest[o] = b.cx;
        closest[o + 1] = b.cy;
        closest[o + 2] = b.cz;
    }
    if (tri) tri[i] = b.tri;
}

// area[t] = 0.5 |e1 x e2| in float64, e1 = p1 - p0 and e2 = p2 - p0 formed in float64 from the
// fp32 vertices of triangle t ([n][9], the caller's order)
__global__ __launch_bounds__(BLOCK) void k_mesh_areas(int n, const float *__restrict__ tris,
                                                      double *__restrict__ area) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float *t = tris + (size_t)9 * i;
    const double e1x = (double)t[3] - (double)t[0], e1y = (double)t[4] - (double)t[1],
                 e1z = (double)t[5] - (double)t[2];
    const double e2x = (double)t[6] - (double)t[0], e2y = (double)t[7] - (double)t[1],
                 e2z = (double)t[8] - (double)t[2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    area[i] = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
}

// splitmix64's output function (Steele, Lea, Flood 2014)
__host__ __device__ __forceinline__ unsigned long long mesh_mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// r_j of sample k in [0, 1): the top 53 bits of
// mix64(mix64(seed + G) + G * (3 k + j + 1)), G = 0x9E3779B97F4A7C15, all modulo 2^64
__device__ __forceinline__ double mesh_uniform(unsigned long long seed_key, int k, int j) {
    const unsigned long long h =
        mesh_mix64(seed_key + 0x9E3779B97F4A7C15ull * (3ull * (unsigned long long)k + (unsigned long long)j + 1ull));
    return (double)(h >> 11) * 0x1.0p-53;
}

// stratified, area-weighted surface samples: sample k sits at x = (k + r0) / n * area of the
// running area and falls into the first triangle t with area_cdf[t] > x
__global__ __launch_bounds__(BLOCK) void k_mesh_sample(int n, int n_tri, const float *__restrict__ tris,
                                                       const double *__restrict__ area_cdf,
                                                       unsigned long long seed_key,
                                                       float *__restrict__ points,
                                                       int32_t *__restrict__ tri) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const double total = area_cdf[n_tri - 1];
    const double r0 = mesh_uniform(seed_key, k, 0), r1 = mesh_uniform(seed_key, k, 1),
                 r2 = mesh_uniform(seed_key, k, 2);
    double x = ((double)k + r0) / (double)n * total;
    // (k + r0) / n may round up to 1: keep x below the total, so that a triangle with
    // area_cdf[t] > x exists (total > 0, the caller's check)
    if (!(x < total)) x = __longlong_as_double(__double_as_longlong(total) - 1);
    int lo = 0, hi = n_tri - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (area_cdf[mid] > x)
            hi = mid;
        else
            lo = mid + 1;
    }
    const float *t = tris + (size_t)9 * lo;
    const bool fold = r1 + r2 > 1.;
    const double u = fold ? 1. - r1 : r1, v = fold ? 1. - r2 : r2;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double p0 = (double)t[c];
        const double e1 = (double)t[3 + c] - p0, e2 = (double)t[6 + c] - p0;
        points[3 * (size_t)k + c] = (float)((p0 + u * e1) + v * e2);
    }
    tri[k] = lo;
}

constexpr int MESH_MAX_TRIANGLES = 1 << 30;

}  // namespace

extern "C" {

int rn_mesh_keys(rn_ctx *ctx, int32_t n, const float *triangles, const float *box,
                 int64_t *keys, void *stream) {
    if (!ctx || n < 1 || n > MESH_MAX_TRIANGLES || !triangles || !box || !keys)
        return fail(ctx, RN_ERR_INVALID, "bad argument");
    hipLaunchKernelGGL(k_mesh_keys, dim3(thread_blocks(n)), dim3(BLOCK), 0, S(stream), n, triangles,
                       box, reinterpret_cast<unsigned long long *>(keys));
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_mesh_build(rn_ctx *ctx, int32_t n, const float *triangles, const int64_t *sorted_keys,
                  float *nodes, float *leaves, void *work, int32_t *depth_out, void *stream) {
    if (!ctx || n < 1 || n > MESH_MAX_TRIANGLES || !triangles || !sorted_keys || !nodes ||
        !leaves || !work || !depth_out)
        return fail(ctx, RN_ERR_INVALID, "bad argument");
    const int n_int = n > 1 ? n - 1 : 1;
    const auto *keys = reinterpret_cast<const unsigned long long *>(sorted_keys);
    char *w = static_cast<char *>(work);
    float4 *leaf_box = reinterpret_cast<float4 *>(w);                       // 32 n bytes
    int4 *ranges = reinterpret_cast<int4 *>(w + 32 * (size_t)n);            // 16 n
    int *parent = reinterpret_cast<int *>(w + 48 * (size_t)n);              // 8 n
    int *depth = reinterpret_cast<int *>(w + 56 * (size_t)n);               // 4
    RN_HIP(ctx, hipMemsetAsync(depth, 0, sizeof(int), S(stream)));
    hipLaunchKernelGGL(k_mesh_leaves, dim3(thread_blocks(n)), dim3(BLOCK), 0, S(stream), n, triangles,
                       keys, reinterpret_cast<MeshLeaf *>(leaves), leaf_box);
    RN_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_mesh_hierarchy, dim3(thread_blocks(n_int)), dim3(BLOCK), 0, S(stream), n,
                       n_int, keys, ranges, parent);
    RN_LAUNCH_CHECK(ctx);
    const int waves_per_block = BLOCK / WAVE;
    hipLaunchKernelGGL(k_mesh_boxes, dim3((n_int + waves_per_block - 1) / waves_per_block),
                       dim3(BLOCK), 0, S(stream), n_int, ranges, leaf_box,
                       reinterpret_cast<MeshNode *>(nodes));
    RN_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_mesh_depth, dim3(thread_blocks(n)), dim3(BLOCK), 0, S(stream), n, n_int,
                       parent, depth);
    RN_LAUNCH_CHECK(ctx);
    int h = 0;
    RN_HIP(ctx, hipMemcpyAsync(&h, depth, sizeof(int), hipMemcpyDeviceToHost, S(stream)));
    RN_HIP(ctx, hipStreamSynchronize(S(stream)));
    *depth_out = h;
    // unique 62-bit keys bound the depth to 63; a deeper tree would overrun the stack
    if (h > MESH_STACK - 1)
        return fail(ctx, RN_ERR_INVALID, "BVH depth %d exceeds the traversal stack (%d)", h,
                    MESH_STACK - 1);
    return RN_OK;
}

int rn_mesh_raycast(rn_ctx *ctx, int32_t n, const float *origins, const float *destinations,
                    const float *nodes, const float *leaves, float *points, int32_t *tri,
                    void *stream) {
    RN_OPEN(ctx, n, all_set(origins, destinations, nodes, leaves, points, tri));
    hipLaunchKernelGGL(k_mesh_raycast, dim3((n + MESH_RAY_BLOCK - 1) / MESH_RAY_BLOCK),
                       dim3(MESH_RAY_BLOCK), 0, S(stream), n, origins, destinations,
                       reinterpret_cast<const MeshNode *>(nodes),
                       reinterpret_cast<const MeshLeaf *>(leaves), points, tri);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_mesh_depthmap(rn_ctx *ctx, int32_t H, int32_t W, const float *P_pinv,
                     const float *camera_center, const float *nodes, const float *leaves,
                     float *depth_map, void *stream) {
    if (!ctx || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30 || !P_pinv ||
        !camera_center || !nodes || !leaves || !depth_map)
        return fail(ctx, RN_ERR_INVALID, "bad argument");
    hipLaunchKernelGGL(k_mesh_depthmap, dim3((H * W + MESH_RAY_BLOCK - 1) / MESH_RAY_BLOCK),
                       dim3(MESH_RAY_BLOCK), 0, S(stream), H, W, P_pinv, camera_center,
                       reinterpret_cast<const MeshNode *>(nodes),
                       reinterpret_cast<const MeshLeaf *>(leaves), depth_map);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_mesh_closest(rn_ctx *ctx, int32_t n, const double *queries, const float *nodes,
                    const float *leaves, double *dist, double *closest, int32_t *tri,
                    void *stream) {
    RN_OPEN(ctx, n, all_set(queries, nodes, leaves, dist));
    hipLaunchKernelGGL(k_mesh_closest, dim3((n + MESH_RAY_BLOCK - 1) / MESH_RAY_BLOCK),
                       dim3(MESH_RAY_BLOCK), 0, S(stream), n, queries,
                       reinterpret_cast<const MeshNode *>(nodes),
                       reinterpret_cast<const MeshLeaf *>(leaves), dist, closest, tri);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_mesh_areas(rn_ctx *ctx, int32_t n, const float *triangles, double *area, void *stream) {
    if (!ctx || n < 1 || n > MESH_MAX_TRIANGLES || !triangles || !area)
        return fail(ctx, RN_ERR_INVALID, "bad argument");
    hipLaunchKernelGGL(k_mesh_areas, dim3(thread_blocks(n)), dim3(BLOCK), 0, S(stream), n, triangles,
                       area);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_mesh_sample(rn_ctx *ctx, int32_t n_samples, int32_t n_triangles, const float *triangles,
                   const double *area_cdf, int64_t seed, float *points, int32_t *tri,
                   void *stream) {
    RN_OPEN(ctx, n_samples, n_triangles >= 1 && n_triangles <= MESH_MAX_TRIANGLES &&
                                all_set(triangles, area_cdf, points, tri));
    const unsigned long long seed_key =
        mesh_mix64((unsigned long long)seed + 0x9E3779B97F4A7C15ull);
    hipLaunchKernelGGL(k_mesh_sample, dim3(thread_blocks(n_samples)), dim3(BLOCK), 0, S(stream),
                       n_samples, n_triangles, triangles, area_cdf, seed_key, points, tri);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
