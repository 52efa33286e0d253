// Gradients of the natural frequencies from the converged mode block (include/trs_modegrad.h): for a simple
// eigenvalue d lambda = phi^T (dK - lambda dM) phi, one pass over the members with the block X that trs_modes_step left
// resident - no solve, no factorisation.
//
//   trs_mg_grad   X, lam (as trs_modes_step left them) -> gA, gE, grho [B][R][nM_max], gxyz [B][R][nJ_max][3],
//                 gmass [B][R][nJ_max]; R = p rows (one per eigenvalue) or, with weights, the one row sum_k w_k (row k)
//
// One work-group of 256 threads per truss, as trs_adjoint_grad and trs_effects_recover:
//   stage   c, len, k / len and mu A rho / 2 of every member into LDS - ONCE per work-group, not once per mode (the
//           sqrt, the divisions and the scattered reads of xyz are what a member costs; EXPERIMENTS R12, R18); nJ, nM
//           trimmed and the end joints clamped to the arrays as trs_col::stage does; the member-end lists of every joint
//           (trs_rec::build_end_lists, sorted by member id; an end outside the truss is on no list)
//   pass    phi_k of as many modes as fit beside the tables (mg_pass: within half a CU's LDS where two fit there),
//           joint layout through free_index, zero at held DOFs and
//           past the truss's own joints
//     members   one thread per member: the table row and E, A, rho in registers, the modes of the pass inside
//     joints    one thread per joint: per mode the sum over its list in member-id order (gxyz) and |phi_j|^2 (gmass)
// The weighted row is carried from mode to mode as acc = fma(w_k, g_k, acc), k ascending, by the one thread that owns the
// entry (through the output itself between two passes): how many modes a pass holds changes no bit.  No floating-point
// atomic, every sum in one fixed order.
#include "../../include/trs_modegrad.h"
#include "../../include/trs_modes.h"
#include "trs_common.h"
#include "trs_lds.h"

namespace {

using namespace trs_rec;

static_assert(TRS_MG_BLOCK == TRS_MODES_BLOCK, "the block of trs_modegrad.h is the one of trs_modes.h");

// LDS tables of one truss
struct MgTables : EndLists {   // (the member-end lists of EVERY joint: trs_recover.h)
    double *cx, *cy, *cz;      // [nM_max] each: direction cosines (0 for a member of zero length)
    double* len;               // [nM_max]  0 for a member of zero length: it gets zeros
    double* kl;                // [nM_max]  (E A / len) / len
    double* mg;                // [nM_max]  mass_scale A rho / 2
    double* phi;               // [pc][3 nJ_max]  the modes of the pass, joint layout
    int2* mends;               // [nM_max]  end joints, clamped
};

template <class Arena>
__host__ __device__ inline MgTables layout(Arena& a, int nJ_max, int nM_max, int pc) {
    MgTables t;
    t.cx = a.template take<double>(nM_max);
    t.cy = a.template take<double>(nM_max);
    t.cz = a.template take<double>(nM_max);
    t.len = a.template take<double>(nM_max);
    t.kl = a.template take<double>(nM_max);
    t.mg = a.template take<double>(nM_max);
    t.phi = a.template take<double>((size_t)pc * 3 * nJ_max);
    t.mends = a.template take<int2>(nM_max);
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    return t;
}

size_t mg_lds(int nJ_max, int nM_max, int pc) {
    return trs_lds::count([&](auto& a) { layout(a, nJ_max, nM_max, pc); });
}

// What the two loops take from phi for member (c0, c1): Dphi, s = c . Dphi and h = |phi_j0|^2 + |phi_j1|^2.  ONE
// function, so the member outputs and gxyz see the same s and h.
struct MemberMode {
    double d[3], s, h;
};
__device__ __forceinline__ MemberMode member_mode(const double* ph, const int2 c, const double cx, const double cy,
                                                  const double cz) {
    MemberMode r;
    const double a0 = ph[3 * c.x], a1 = ph[3 * c.x + 1], a2 = ph[3 * c.x + 2];
    const double b0 = ph[3 * c.y], b1 = ph[3 * c.y + 1], b2 = ph[3 * c.y + 2];
    r.d[0] = b0 - a0;
    r.d[1] = b1 - a1;
    r.d[2] = b2 - a2;
    r.s = fma(cz, r.d[2], fma(cy, r.d[1], cx * r.d[0]));
    r.h = fma(a2, a2, fma(a1, a1, a0 * a0)) + fma(b2, b2, fma(b1, b1, b0 * b0));
    return r;
}

__global__ __launch_bounds__(256) void trs_mg_grad_kernel(
    const TrsBatch bt, const double* __restrict__ X_all, const double* __restrict__ lam_all,
    const int* __restrict__ n_mass, const int p, const int pc, const double mass_scale, const double* __restrict__ w_all,
    double* __restrict__ gA, double* __restrict__ gE, double* __restrict__ grho, double* __restrict__ gxyz,
    double* __restrict__ gmass) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max, ld_f = bt.ld_f;
    const int joints = v.joints, members = v.members, ndof_max = v.ndof_max;
    const size_t mbase = v.mbase;
    const TrsMembers& mem = v.mem;
    const int n_modes = min(p, max(n_mass[b], 0));
    const bool weighted = w_all != nullptr;
    const int R = weighted ? 1 : p;
    trs_lds::Carve lds(sh);
    const MgTables t = layout(lds, nJ_max, nM_max, pc);
    const double* Xb = X_all + (size_t)b * TRS_MG_BLOCK * ld_f;
    const double* lam = lam_all + (size_t)b * TRS_MG_BLOCK;
    const double* w = weighted ? w_all + (size_t)b * p : nullptr;
    const bool want_members = (gA != nullptr) | (gE != nullptr) | (grho != nullptr);
    const bool want_joints = (gxyz != nullptr) | (gmass != nullptr);

    // ---- the rows without an eigenvalue: zeros (the whole weighted row when the truss has no mode at all)
    for (int r = weighted ? min(n_modes, 1) : n_modes; r < R; ++r) {
        const size_t row = (size_t)b * R + r;
        for (int m = tid; m < nM_max; m += 256) {
            if (gA != nullptr) gA[row * nM_max + m] = 0.0;
            if (gE != nullptr) gE[row * nM_max + m] = 0.0;
            if (grho != nullptr) grho[row * nM_max + m] = 0.0;
        }
        if (gxyz != nullptr)
            for (int d = tid; d < ndof_max; d += 256) gxyz[row * ndof_max + d] = 0.0;
        if (gmass != nullptr)
            for (int j = tid; j < nJ_max; j += 256) gmass[row * nJ_max + j] = 0.0;
    }
    if (n_modes == 0) return;   // (the whole work-group)

    // ---- stage: the member table, once
    for (int m = tid; m < members; m += 256) {
        const int2 c = v.ends(m).c;
        const MemberGeom g = member_geom(v.X, c.x, c.y);
        const bool live = g.len > 0.0;
        t.mends[m] = c;
        t.cx[m] = live ? g.c[0] : 0.0;
        t.cy[m] = live ? g.c[1] : 0.0;
        t.cz[m] = live ? g.c[2] : 0.0;
        t.len[m] = live ? g.len : 0.0;
        t.kl[m] = live ? mem.EA(mbase + m) / g.len / g.len : 0.0;
        t.mg[m] = live ? mass_scale * (0.5 * (mem.area(mbase + m) * mem.density(mbase + m))) : 0.0;
    }
    if (gxyz != nullptr) build_end_lists(t, v, tid);

    for (int k0 = 0; k0 < n_modes; k0 += pc) {
        const int kc = min(pc, n_modes - k0);
        __syncthreads();   // (the tables and the lists are written; the previous pass's readers of phi are done)
        for (int x = tid; x < kc * ndof_max; x += 256) {
            const int kk = x / ndof_max, d = x - kk * ndof_max;
            const int row = v.row_of(d);
            t.phi[x] = row >= 0 ? Xb[(size_t)(k0 + kk) * ld_f + row] : 0.0;
        }
        __syncthreads();

        // ---- members: gA, gE, grho
        if (want_members)
            for (int m = tid; m < nM_max; m += 256) {
                const bool live = m < members && t.len[m] > 0.0;
                int2 c = int2{0, 0};
                double cx = 0.0, cy = 0.0, cz = 0.0, ke = 0.0, ka = 0.0, mh = 0.0, mr = 0.0;
                if (live) {
                    c = t.mends[m];
                    cx = t.cx[m], cy = t.cy[m], cz = t.cz[m];
                    const double len = t.len[m], a = mem.area(mbase + m), rho = mem.density(mbase + m);
                    ke = modulus(mem, mbase + m) / len;
                    ka = a / len;
                    mh = mass_scale * (0.5 * (len * rho));
                    mr = mass_scale * (0.5 * (a * len));
                }
                double accA = 0.0, accE = 0.0, accR = 0.0;
                if (weighted && k0 > 0) {   // this thread's own entries of the pass before
                    if (gA != nullptr) accA = gA[(size_t)b * nM_max + m];
                    if (gE != nullptr) accE = gE[(size_t)b * nM_max + m];
                    if (grho != nullptr) accR = grho[(size_t)b * nM_max + m];
                }
                for (int kk = 0; kk < kc; ++kk) {
                    double vA = 0.0, vE = 0.0, vR = 0.0;
                    if (live) {
                        const double l = lam[k0 + kk];
                        const MemberMode q = member_mode(t.phi + (size_t)kk * ndof_max, c, cx, cy, cz);
                        const double s2 = q.s * q.s, lh = l * q.h;
                        vA = ke * s2 - lh * mh;
                        vE = ka * s2;
                        vR = -(lh * mr);
                    }
                    if (weighted) {
                        const double wk = w[k0 + kk];
                        accA = fma(wk, vA, accA);
                        accE = fma(wk, vE, accE);
                        accR = fma(wk, vR, accR);
                    } else {
                        const size_t o = ((size_t)b * p + k0 + kk) * nM_max + m;
                        if (gA != nullptr) gA[o] = vA;
                        if (gE != nullptr) gE[o] = vE;
                        if (grho != nullptr) grho[o] = vR;
                    }
                }
                if (weighted) {
                    if (gA != nullptr) gA[(size_t)b * nM_max + m] = live ? accA : 0.0;
                    if (gE != nullptr) gE[(size_t)b * nM_max + m] = live ? accE : 0.0;
                    if (grho != nullptr) grho[(size_t)b * nM_max + m] = live ? accR : 0.0;
                }
            }

        // ---- joints: gxyz (the sum over the joint's list, member-id order) and gmass
        if (want_joints)
            for (int j = tid; j < nJ_max; j += 256) {
                const bool own = j < joints;
                const int o = v.place(j);
                const int* list = t.ends + (own && gxyz != nullptr ? t.start[j] : 0);
                const int deg = own && gxyz != nullptr ? t.cnt[j] : 0;
                double acc[3] = {0.0, 0.0, 0.0}, accM = 0.0;
                if (weighted && k0 > 0) {
                    if (gxyz != nullptr) {
#pragma unroll
                        for (int a = 0; a < 3; ++a) acc[a] = gxyz[((size_t)b * nJ_max + o) * 3 + a];
                    }
                    if (gmass != nullptr) accM = gmass[(size_t)b * nJ_max + o];
                }
                for (int kk = 0; kk < kc; ++kk) {
                    const double* ph = t.phi + (size_t)kk * ndof_max;
                    const double l = lam[k0 + kk];
                    double r[3] = {0.0, 0.0, 0.0};
                    for (int i = 0; i < deg; ++i) {
                        const int m = list[i] >> 1, end = list[i] & 1;
                        const double cm[3] = {t.cx[m], t.cy[m], t.cz[m]};
                        const MemberMode q = member_mode(ph, t.mends[m], cm[0], cm[1], cm[2]);
                        const double ks = t.kl[m] * q.s, s3 = 3.0 * q.s, lm = l * t.mg[m] * q.h;
                        double gm[3];
#pragma unroll
                        for (int a = 0; a < 3; ++a) gm[a] = ks * (2.0 * q.d[a] - s3 * cm[a]) - lm * cm[a];
                        add_end_force(r, gm, 1.0, end);
                    }
                    double vM = 0.0;
                    if (own) {
                        const double p0 = ph[3 * j], p1 = ph[3 * j + 1], p2 = ph[3 * j + 2];
                        vM = -(l * fma(p2, p2, fma(p1, p1, p0 * p0)));
                    }
                    if (weighted) {
                        const double wk = w[k0 + kk];
#pragma unroll
                        for (int a = 0; a < 3; ++a) acc[a] = fma(wk, r[a], acc[a]);
                        accM = fma(wk, vM, accM);
                    } else {
                        const size_t row = (size_t)b * p + k0 + kk;
                        if (gxyz != nullptr) {
#pragma unroll
                            for (int a = 0; a < 3; ++a) gxyz[(row * nJ_max + o) * 3 + a] = own ? r[a] : 0.0;
                        }
                        if (gmass != nullptr) gmass[row * nJ_max + o] = vM;
                    }
                }
                if (weighted) {
                    if (gxyz != nullptr) {
#pragma unroll
                        for (int a = 0; a < 3; ++a) gxyz[((size_t)b * nJ_max + o) * 3 + a] = own ? acc[a] : 0.0;
                    }
                    if (gmass != nullptr) gmass[(size_t)b * nJ_max + o] = own ? accM : 0.0;
                }
            }
    }
}

// Modes per pass (0 = none fit): the most that fit a CU's LDS - but where at least two modes per pass fit HALF of it, no
// more than that, so that two work-groups share a CU and hide each other's staging latency (bar-942, p = 8: three modes per
// pass in 79 824 B, 0.83 ms for 4096 trusses against 1.22 ms with all eight in 109 104 B; EXPERIMENTS R22).  The weighted
// row is carried in mode order whatever a pass holds, so the choice changes no bit.
int mg_pass(int nJ_max, int nM_max, int p) {
    int pc = p;
    while (pc > 0 && mg_lds(nJ_max, nM_max, pc) > TRS_LDS_BYTES) --pc;
    int half = pc;
    while (half > 0 && mg_lds(nJ_max, nM_max, half) > TRS_LDS_BYTES / 2) --half;
    return half >= 2 ? half : pc;
}

int mg_launch(int B, const TrsBatch& bt, const double* X, const double* lam, const int* n_mass, int p, double mass_scale,
              const double* w, double* gA, double* gE, double* grho, double* gxyz, double* gmass, hipStream_t stream) {
    if (B <= 0) return 0;
    if (!trs_mg_fits(bt.nJ_max, bt.nM_max, p) || bt.ld_f < 1 || X == nullptr || lam == nullptr || n_mass == nullptr)
        return (int)hipErrorInvalidValue;
    if (gA == nullptr && gE == nullptr && grho == nullptr && gxyz == nullptr && gmass == nullptr) return 0;
    const int pc = mg_pass(bt.nJ_max, bt.nM_max, p);
    trs_lds::raise_lds_once<trs_mg_grad_kernel>();
    hipLaunchKernelGGL(trs_mg_grad_kernel, dim3(B), dim3(256), mg_lds(bt.nJ_max, bt.nM_max, pc), stream, bt, X, lam, n_mass,
                       p, pc, mass_scale, w, gA, gE, grho, gxyz, gmass);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_mg_abi_version(void) { return TRS_MG_ABI_VERSION; }

int trs_mg_fits(int nJ_max, int nM_max, int p) {
    return nJ_max >= 0 && nM_max >= 0 && p >= 1 && p <= TRS_MG_MAX_MODES && mg_lds(nJ_max, nM_max, 1) <= TRS_LDS_BYTES;
}

int trs_mg_grad(int B, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E, const double* A,
                const double* rho, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                const int32_t* nM, const int32_t* joint_out, const double* X, int ld_f, const double* lam,
                const int32_t* n_mass, int p, double mass_scale, const double* w, double* gA, double* gE, double* grho,
                double* gxyz, double* gmass, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A, rho), free_index, n_free, nJ, nM,
                                  joint_out, ld_f);
    return mg_launch(B, bt, X, lam, n_mass, p, mass_scale, w, gA, gE, grho, gxyz, gmass, (hipStream_t)stream);
}

int trs_mg_tab_grad(int B, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16, const uint8_t* type_idx,
                    const double* types, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                    const int32_t* nM, const int32_t* joint_out, const double* X, int ld_f, const double* lam,
                    const int32_t* n_mass, int p, double mass_scale, const double* w, double* gA, double* gE,
                    double* grho, double* gxyz, double* gmass, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free, nJ,
                                  nM, joint_out, ld_f);
    return mg_launch(B, bt, X, lam, n_mass, p, mass_scale, w, gA, gE, grho, gxyz, gmass, (hipStream_t)stream);
}

}  // extern "C"
