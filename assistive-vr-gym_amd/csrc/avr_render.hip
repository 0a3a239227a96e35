// avr_render.hip -- ray-cast views of the envs' collision geometry on the device (include/avr.h
// avr_render_device, avr_get_body_poses): depth, shape id and a shaded RGB image per rendered env.
// Read-only: nothing here writes the state, the workspace, the collision scratch or a graph.
// Included once per task inside the task's namespace (avr_task_tu.h) after avr_trainstats.hip.
//
// Two launches per call:
//   1. avr_render_frames_kernel   one wavefront per rendered env.  The body COM frames of the env's
//      current state by the pair kernel's own device code (load_state, robot_fk, body_tf: what fills
//      CS_BTF at the start of a sub-step), then one record per shape into the handle's render scratch:
//      the shape's world frame, its parameters, a bounding radius about the frame's origin (a hull's comes from the host) and its
//      kind (-1: the other gender's shape).  Lane 0 resolves the camera (a body-attached one through
//      that body's frame) into eye, right, up, forward.  avr_get_body_poses is this kernel with the
//      frames copied out instead.
//   2. avr_render_trace_kernel    one wavefront per 8 x 8 pixel tile of one env, lane = pixel.
//      Prologue: the lanes stride over the env's shape records, test each bounding sphere against the
//      tile's four side planes (planes through the eye, in camera coordinates) and the [near, far]
//      shell, and compact the survivors with ballots into an LDS list -- ascending shape order, no
//      atomics.  Then every lane traces its pixel through the list: the list entry, the shape record
//      and a hull's planes are read at wave-uniform addresses (readfirstlane), so the per-lane state
//      is the ray, the running best (t, id, local normal) and the current shape's interval.
//      Sphere, capsule (cylinder + two caps) and box (slabs) are closed forms in the shape's frame; a
//      hull clips the ray's interval against its face planes (avr_render_set_planes).
// A hit is where the ray ENTERS a shape (the surface faces the ray) with t in [near, far]: a shape
// that holds the eye, or that the near distance cuts, is not seen, as a back-face-culling rasteriser
// would not see it.  Ties between shapes go to the lower index (the list is ascending, the update is
// a strict <).
// Arithmetic: fp contract(off) with no fused operation, so an image does not change with unrelated
// edits; sqrtf and / are IEEE.

#define RD_TILE 8                                 // a tile is RD_TILE x RD_TILE pixels = one wavefront
#define RD_CAM_WORDS 16                           // resolved camera: eye3, right3, up3, forward3, pad
#define RD_REC_WORDS 12                           // shape record: p3, q4, param3, bounding radius, kind (int bits)
#define RD_MAX_DIM 4096
static_assert(RD_TILE * RD_TILE == 64, "one lane per pixel of a tile");
static_assert(RD_CAM_WORDS % 4 == 0 && RD_REC_WORDS % 4 == 0, "records are read as float4");

// avr_camera with the derived pixel scale, by value in the kernel arguments
struct RdCam {
    float eye[3], target[3], up[3];
    float th_h;                 // tan(fov_y / 2) / height: x = (2 c + 1 - W) th_h, y = (H - 2 r - 1) th_h
    float near, far;
    int W, H, body;
};

AVR_DI size_t rd_stride(int ns) { return (size_t)RD_CAM_WORDS + (size_t)RD_REC_WORDS * ns; }

AVR_DI v3 rd_add(v3 a, v3 b) {
#pragma clang fp contract(off)
    return V(a.x + b.x, a.y + b.y, a.z + b.z);
}
AVR_DI v3 rd_sub(v3 a, v3 b) {
#pragma clang fp contract(off)
    return V(a.x - b.x, a.y - b.y, a.z - b.z);
}
AVR_DI v3 rd_scl(v3 a, float s) {
#pragma clang fp contract(off)
    return V(a.x * s, a.y * s, a.z * s);
}
AVR_DI float rd_dot(v3 a, v3 b) {
#pragma clang fp contract(off)
    return (a.x * b.x + a.y * b.y) + a.z * b.z;
}
AVR_DI v3 rd_crs(v3 a, v3 b) {
#pragma clang fp contract(off)
    return V(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
AVR_DI v3 rd_unit(v3 a) {
#pragma clang fp contract(off)
    const float n = sqrtf(rd_dot(a, a));
    return V(a.x / n, a.y / n, a.z / n);
}
// v rotated by q: v + w t + u x t, t = 2 u x v
AVR_DI v3 rd_rot(qt q, v3 v) {
#pragma clang fp contract(off)
    const v3 u = V(q.x, q.y, q.z);
    const v3 t = rd_scl(rd_crs(u, v), 2.0f);
    return rd_add(rd_add(v, rd_scl(t, q.w)), rd_crs(u, t));
}
AVR_DI qt rd_qmul(qt a, qt b) {
#pragma clang fp contract(off)
    return Q(((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y, ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x,
             ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w, ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z);
}

// ------------------------------------------------------------------ launch 1: frames
// Grid: one 64-lane block per rendered env (slot = blockIdx.x; env = env_ids[slot], NULL: slot).
// scr (may be NULL): the slot's camera and shape records.  poses (may be NULL): [slot][nb][7].
// hull_radius [ns]: the largest |vertex| of each hull shape (0 for the other kinds).
__global__ __launch_bounds__(64) void avr_render_frames_kernel(const KModel *__restrict__ mp, const float *__restrict__ state,
                                                               const int *__restrict__ env_ids, int n_envs, const RdCam cam,
                                                               const float *__restrict__ hull_radius, float *__restrict__ scr,
                                                               float *__restrict__ poses) {
#pragma clang fp contract(off)
    __shared__ PairsLDS L;
    const KModel &m = *mp;
    const int slot = blockIdx.x, lane = lane_id();
    const int env = min(max(env_ids ? env_ids[slot] : slot, 0), n_envs - 1);   // (validated on the host; never an index outside the state)
    load_state(m, L, state + (size_t)env * K_STATE_WORDS);
    const int gender = L.gender;
    const int vso = lvrow(L, m) * m.ns;
    robot_fk(m, L);
    if (lane < m.nb) {
        const tf t = body_tf(m, L, lane);
        sttf(L.btf[lane], t);
        if (poses) {
            float *o = poses + ((size_t)slot * m.nb + lane) * 7;
            o[0] = t.p.x; o[1] = t.p.y; o[2] = t.p.z; o[3] = t.q.x; o[4] = t.q.y; o[5] = t.q.z; o[6] = t.q.w;
        }
    }
    SYNC();
    if (!scr) return;
    float *out = scr + (size_t)slot * rd_stride(m.ns);
    if (lane == 0) {
        v3 eye = V(cam.eye[0], cam.eye[1], cam.eye[2]), tgt = V(cam.target[0], cam.target[1], cam.target[2]), up = V(cam.up[0], cam.up[1], cam.up[2]);
        if (cam.body >= 0) {
            const tf T = ldtf(L.btf[min(cam.body, m.nb - 1)]);
            eye = rd_add(T.p, rd_rot(T.q, eye));
            tgt = rd_add(T.p, rd_rot(T.q, tgt));
            up = rd_rot(T.q, up);
        }
        const v3 f = rd_unit(rd_sub(tgt, eye));
        const v3 r = rd_unit(rd_crs(f, up));
        const v3 u = rd_crs(r, f);
        st3(out, eye); st3(out + 3, r); st3(out + 6, u); st3(out + 9, f);
        out[12] = 0.f; out[13] = 0.f; out[14] = 0.f; out[15] = 0.f;
    }
    for (int s = lane; s < m.ns; s += 64) {
        const int kind = gld(m.shape_kind + s);
        const int g = gld(m.shape_gender + s);
        const tf B = ldtf(L.btf[min(max(gld(m.shape_body + s), 0), m.nb - 1)]);
        const tf P = gldtf(m.shape_pose + 8 * (s + vso));
        const v3 p = rd_add(B.p, rd_rot(B.q, P.p));
        const qt q = rd_qmul(B.q, P.q);
        const v3 pa = gld3(m.shape_param + 4 * (s + vso));
        float br;
        if (kind == AVR_SPHERE) br = pa.x;
        else if (kind == AVR_CAPSULE) br = pa.x + pa.y;
        else if (kind == AVR_BOX) br = sqrtf(rd_dot(pa, pa));
        else br = gld(hull_radius + s);     // (constant per scene: avr_create computes it once)
        float4 *o = (float4 *)(out + RD_CAM_WORDS + RD_REC_WORDS * s);
        o[0] = make_float4(p.x, p.y, p.z, q.x);
        o[1] = make_float4(q.y, q.z, q.w, pa.x);
        o[2] = make_float4(pa.y, pa.z, br, __int_as_float((g < 0 || g == gender) ? kind : -1));
    }
}

// ------------------------------------------------------------------ launch 2: trace
// the entering hit of one convex shape in its own frame: t (+inf: none) and the outward normal there
struct RdHit { float t; v3 n; };

// |o + t d| = r, the smaller root, through the ray's point of closest approach (no cancellation
// between |o|^2 and r^2 for a small sphere far away)
AVR_DI float rd_sphere_t(v3 o, v3 d, float r) {
#pragma clang fp contract(off)
    const float tc = -rd_dot(o, d);
    const v3 mm = rd_add(o, rd_scl(d, tc));
    const float disc = r * r - rd_dot(mm, mm);
    return disc >= 0.f ? tc - sqrtf(disc) : INFINITY;
}

AVR_DI RdHit rd_sphere(v3 o, v3 d, float r) {
#pragma clang fp contract(off)
    RdHit h;
    h.t = rd_sphere_t(o, d, r);
    h.n = rd_scl(rd_add(o, rd_scl(d, h.t)), 1.0f / r);
    return h;
}

// capsule along z: radius r, half height hh
AVR_DI RdHit rd_capsule(v3 o, v3 d, float r, float hh) {
#pragma clang fp contract(off)
    RdHit h;
    h.t = INFINITY; h.n = V(0, 0, 0);
    const float a = d.x * d.x + d.y * d.y;
    if (a > 1e-12f) {
        const float tc = -(o.x * d.x + o.y * d.y) / a;
        const float mx = o.x + tc * d.x, my = o.y + tc * d.y;
        const float disc = r * r - (mx * mx + my * my);
        if (disc >= 0.f) {
            const float t = tc - sqrtf(disc / a);
            const float z = o.z + t * d.z;
            if (fabsf(z) <= hh) { h.t = t; h.n = V((o.x + t * d.x) / r, (o.y + t * d.y) / r, 0.f); }
        }
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float cz = k ? -hh : hh;
        const v3 oc = V(o.x, o.y, o.z - cz);
        const float t = rd_sphere_t(oc, d, r);
        const float z = oc.z + t * d.z;
        if (t < h.t && (k ? z <= 0.f : z >= 0.f)) { h.t = t; h.n = rd_scl(rd_add(oc, rd_scl(d, t)), 1.0f / r); }
    }
    return h;
}

// box of half extents he: slabs
AVR_DI RdHit rd_box(v3 o, v3 d, v3 he) {
#pragma clang fp contract(off)
    RdHit h;
    float tmin = -INFINITY, tmax = INFINITY;
    v3 nn = V(0, 0, 0);
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, hh[3] = {he.x, he.y, he.z};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (dd[i] == 0.f) {
            if (fabsf(oo[i]) > hh[i]) tmax = -INFINITY;
        } else {
            const float t1 = (-hh[i] - oo[i]) / dd[i], t2 = (hh[i] - oo[i]) / dd[i];
            const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
            if (lo > tmin) {
                const float sg = dd[i] > 0.f ? -1.f : 1.f;
                tmin = lo;
                nn = V(i == 0 ? sg : 0.f, i == 1 ? sg : 0.f, i == 2 ? sg : 0.f);
            }
            tmax = fminf(tmax, hi);
        }
    }
    h.t = tmin <= tmax ? tmin : INFINITY;
    h.n = nn;
    return h;
}

// convex hull as planes n . x <= w (pl[k] = (n, w), the same address in every lane): the ray's
// interval clipped plane by plane
AVR_DI RdHit rd_hull(v3 o, v3 d, const float4 *__restrict__ pl, int np) {
#pragma clang fp contract(off)
    RdHit h;
    float tmin = -INFINITY, tmax = INFINITY;
    v3 nn = V(0, 0, 0);
    for (int k = 0; k < np; k++) {
        const float4 P = gld(pl + k);
        const v3 n = V(P.x, P.y, P.z);
        const float den = rd_dot(n, d), dist = P.w - rd_dot(n, o);
        if (den < 0.f) {
            const float t = dist / den;
            if (t > tmin) { tmin = t; nn = n; }
        } else if (den > 0.f) {
            tmax = fminf(tmax, dist / den);
        } else if (dist < 0.f) {
            tmax = -INFINITY;
        }
    }
    h.t = (np > 0 && tmin <= tmax) ? tmin : INFINITY;
    h.n = nn;
    return h;
}

// Grid: (tiles_x * tiles_y, n).  scr: launch 1's output.  Any of depth / id / rgb may be NULL.  stats (may be
// NULL; avr_render_tile_stats): per tile {shapes in its culled list, hull planes a pixel of it tests}.
__global__ __launch_bounds__(64) void avr_render_trace_kernel(const KModel *__restrict__ mp, const float *__restrict__ scr, const RdCam cam,
                                                              const float4 *__restrict__ planes, const int2 *__restrict__ prange, int tiles_x,
                                                              float *__restrict__ depth, int *__restrict__ id, unsigned char *__restrict__ rgb,
                                                              int *__restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ unsigned short list[MAXSH];
    const KModel &m = *mp;
    const int lane = lane_id(), slot = blockIdx.y;
    const int ns = min(m.ns, MAXSH);
    const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
    const float *__restrict__ cw = scr + (size_t)slot * rd_stride(m.ns);
    const float *__restrict__ rec = cw + RD_CAM_WORDS;
    const v3 eye = gld3(cw), ex = gld3(cw + 3), ey = gld3(cw + 6), ez = gld3(cw + 9);

    // prologue: the shapes whose bounding sphere meets the tile's pyramid between near and far
    const int c0 = RD_TILE * tx, r0 = RD_TILE * ty;
    const float xl = (float)(2 * c0 - cam.W) * cam.th_h, xr = (float)(2 * (c0 + RD_TILE) - cam.W) * cam.th_h;
    const float yt = (float)(cam.H - 2 * r0) * cam.th_h, yb = (float)(cam.H - 2 * (r0 + RD_TILE)) * cam.th_h;
    const float il = 1.0f / sqrtf(1.0f + xl * xl), ir = 1.0f / sqrtf(1.0f + xr * xr);
    const float it = 1.0f / sqrtf(1.0f + yt * yt), ib = 1.0f / sqrtf(1.0f + yb * yb);
    int cnt = 0;
    for (int b = 0; b < ns; b += 64) {
        const int s = b + lane, sc = min(s, ns - 1);
        const float4 a0 = gld((const float4 *)(rec + RD_REC_WORDS * sc));
        const float4 a2 = gld((const float4 *)(rec + RD_REC_WORDS * sc) + 2);
        const v3 c = rd_sub(V(a0.x, a0.y, a0.z), eye);
        const float cx = rd_dot(c, ex), cy = rd_dot(c, ey), cz = rd_dot(c, ez);
        const float dist = sqrtf(rd_dot(c, c));
        const float R = a2.z + 1e-4f * (1.0f + dist);      // (slack: the test runs in fp32; culling must never drop a shape a ray can hit)
        bool keep = s < ns && __float_as_int(a2.w) >= 0;
        keep = keep && (xl * cz - cx) * il <= R && (cx - xr * cz) * ir <= R && (cy - yt * cz) * it <= R && (yb * cz - cy) * ib <= R;
        keep = keep && dist - R <= cam.far && dist + R >= cam.near;
        int tot;
        const int pre = ballot_prefix(keep, &tot);
        if (keep) list[cnt + pre] = (unsigned short)s;
        cnt += tot;
    }
    SYNC();

    // the lane's ray
    const int pc = c0 + (lane & (RD_TILE - 1)), pr = r0 + (lane >> 3);
    const float px = (float)(2 * pc + 1 - cam.W) * cam.th_h, py = (float)(cam.H - 2 * pr - 1) * cam.th_h;
    const v3 d = rd_unit(rd_add(ez, rd_add(rd_scl(ex, px), rd_scl(ey, py))));
    float best = INFINITY;
    int bid = -1;
    v3 bn = V(0, 0, 0);
    int npl = 0;
    for (int k = 0; k < cnt; k++) {
        const int s = __builtin_amdgcn_readfirstlane((int)list[k]);
        const float4 *__restrict__ R4 = (const float4 *)(rec + RD_REC_WORDS * s);
        const float4 a0 = gld(R4), a1 = gld(R4 + 1), a2 = gld(R4 + 2);
        const int kind = __float_as_int(a2.w);
        const qt qc = Q(-a0.w, -a1.x, -a1.y, a1.z);
        const v3 o = rd_rot(qc, rd_sub(eye, V(a0.x, a0.y, a0.z))), dl = rd_rot(qc, d);
        RdHit h;
        if (kind == AVR_SPHERE) h = rd_sphere(o, dl, a1.w);
        else if (kind == AVR_CAPSULE) h = rd_capsule(o, dl, a1.w, a2.x);
        else if (kind == AVR_BOX) h = rd_box(o, dl, V(a1.w, a2.x, a2.y));
        else {
            const int2 pr2 = gld(prange + s);
            h = rd_hull(o, dl, planes + pr2.x, pr2.y);
            npl += pr2.y;
        }
        if (h.t >= cam.near && h.t <= cam.far && h.t < best) { best = h.t; bid = s; bn = h.n; }
    }
    if (stats && lane == 0) {
        int *o = stats + 2 * ((size_t)slot * gridDim.x + blockIdx.x);
        o[0] = cnt; o[1] = npl;
    }
    if (pc >= cam.W || pr >= cam.H) return;
    const size_t pix = ((size_t)slot * cam.H + pr) * cam.W + pc;
    if (depth) depth[pix] = best;
    if (id) id[pix] = bid;
    if (rgb) {
        float cr = 204.f, cg = 230.f, cb = 255.f;
        if (bid >= 0) {
            const float4 a0 = gld((const float4 *)(rec + RD_REC_WORDS * bid)), a1 = gld((const float4 *)(rec + RD_REC_WORDS * bid) + 1);
            const v3 nw = rd_rot(Q(a0.w, a1.x, a1.y, a1.z), bn);
            const float shade = 0.3f + 0.7f * fmaxf(0.f, -rd_dot(nw, d));
            const int bk = gld(m.body_kind + min(max(gld(m.shape_body + bid), 0), m.nb - 1));
            // palette by body kind: robot (and robot-fixed), tool / free, human, static
            if (bk == AVR_BODY_ROBOT || bk == AVR_BODY_RSTATIC) { cr = 190.f; cg = 195.f; cb = 205.f; }
            else if (bk == AVR_BODY_FREE) { cr = 240.f; cg = 200.f; cb = 60.f; }
            else if (bk == AVR_BODY_HUMAN) { cr = 230.f; cg = 170.f; cb = 140.f; }
            else { cr = 140.f; cg = 150.f; cb = 160.f; }
            cr = rintf(cr * shade); cg = rintf(cg * shade); cb = rintf(cb * shade);
        }
        unsigned char *o = rgb + 3 * pix;
        o[0] = (unsigned char)fminf(cr, 255.f); o[1] = (unsigned char)fminf(cg, 255.f); o[2] = (unsigned char)fminf(cb, 255.f);
    }
}

hipError_t avr_launch_render_frames(const KModel *d_m, const float *state, const int *d_env_ids, int n, int n_envs, const RdCam &cam,
                                    const float *hull_radius, float *scr, float *poses, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(avr_render_frames_kernel, dim3(n), dim3(64), 0, st, d_m, state, d_env_ids, n_envs, cam, hull_radius, scr, poses);
    return hipGetLastError();
}

hipError_t avr_launch_render_trace(const KModel *d_m, const float *scr, int n, const RdCam &cam, const float4 *planes, const int2 *prange,
                                   float *depth, int *id, unsigned char *rgb, int *stats, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int tiles_x = (cam.W + RD_TILE - 1) / RD_TILE, tiles_y = (cam.H + RD_TILE - 1) / RD_TILE;
    hipLaunchKernelGGL(avr_render_trace_kernel, dim3(tiles_x * tiles_y, n), dim3(64), 0, st, d_m, scr, cam, planes, prange, tiles_x, depth, id, rgb,
                       stats);
    return hipGetLastError();
}

hipError_t avr_render_attrs(int *out8) {
    const void *k[2] = {(const void *)avr_render_frames_kernel, (const void *)avr_render_trace_kernel};
    for (int i = 0; i < 2; i++) {
        hipFuncAttributes a;
        hipError_t e = hipFuncGetAttributes(&a, k[i]);
        if (e != hipSuccess) return e;
        out8[4 * i + 0] = a.numRegs; out8[4 * i + 1] = 0; out8[4 * i + 2] = (int)a.sharedSizeBytes; out8[4 * i + 3] = (int)a.localSizeBytes;
    }
    return hipSuccess;
}
