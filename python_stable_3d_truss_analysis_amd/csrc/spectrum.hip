// Response spectrum analysis from the converged mode block (include/trs_spectrum.h): participation factors, spectral
// ordinates and the peak displacements, member forces and reactions combined over the modes by SRSS, CQC or absolute
// sum, with the block X that trs_modes_step left resident and - for the missing-mass correction - one more substitution
// against the resident factor (trs_potrs_cases, unchanged, between the two kernels).
//
//   trs_rs_modal     X, lam, Mf -> gamma, sa, meff [B][G][p], mtot, base [B][G], the amplitudes q [B][G][p], the
//                    correlations rho [B][8][8] and, with missing mass, the pseudo-static loads in F [B][16][ld_f]
//   trs_rs_combine   X, q, rho (and the solved F) -> u, R [B][G][nJ_max][3], N [B][G][nM_max] and the signed modal values
//
// Both are one work-group of 256 threads per truss.  trs_rs_modal walks the DOFs in joint layout (free_index gives the
// reduced row, d % 3 the axis): a strided partial per thread, a butterfly inside the wave, the four waves in order.
// trs_rs_combine stages ALL response vectors of the truss in LDS in joint layout (the p mode shapes once, the G
// missing-mass solutions behind them); then
//   members   one thread per member, visited once: geometry and E A in registers, the axial value of every mode formed
//             once and scaled by q per direction - up to nine modal values in registers, compile-time indexed
//   joints    one thread per joint: u per direction and component; for a joint with a held DOF the thread walks the
//             joint's member-end list in member-id order (trs_rec::build_end_lists) for R
// No floating-point atomic, every sum in one fixed order.  member_axials / member_modal and combine are the ONE function
// each that the member pass, the reaction pass and the base shear share.  The walk over the DOFs, the reduction, the
// stage, the member and the end forces of a joint are the ones of harmonic.hip: trs_modal.h.
#include "trs_modal.h"

namespace {

using namespace trs_rec;
using namespace trs_modal;

constexpr int DIRS = TRS_RS_MAX_DIRS;

// LDS of the combine kernel
struct RsTables : EndLists {   // (the member-end lists of every joint of the truss: trs_recover.h)
    double* vec;               // [nvec][3 nJ_max]  the response vectors, joint layout: modes 0 .. p - 1, then direction g's
                               //                   missing-mass solution at p + g
    double* rho;               // [8][8]            the correlations of the modes
    double* q;                 // [3][8]            the amplitudes, 0 where there is none
};

template <class Arena>
__host__ __device__ inline RsTables layout(Arena& a, int nJ_max, int nM_max, int nvec) {
    RsTables t;
    t.vec = a.template take<double>((size_t)nvec * 3 * nJ_max);
    t.rho = a.template take<double>(MODES * MODES);
    t.q = a.template take<double>(DIRS * MODES);
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    return t;
}

size_t rs_lds(int nJ_max, int nM_max, int nvec) {
    return trs_lds::count([&](auto& a) { layout(a, nJ_max, nM_max, nvec); });
}

// The combination of the nine slots r (modes 0 .. 7, missing mass at 8; a slot without a response holds 0) under `rule`;
// rho [8][8] in LDS.  i ascending, j ascending inside it; SRSS sums the diagonal only.
__device__ __forceinline__ double combine(const double* rho, const double (&r)[VEC], const int rule) {
    double s = 0.0;
    if (rule == TRS_RS_ABS) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s += fabs(r[i]);
        return s;
    }
    if (rule == TRS_RS_CQC) {
#pragma unroll
        for (int i = 0; i < MODES; ++i) {
#pragma unroll
            for (int j = 0; j < MODES; ++j) s = fma(rho[i * MODES + j] * r[i], r[j], s);
        }
    } else {
#pragma unroll
        for (int i = 0; i < MODES; ++i) s = fma(r[i], r[i], s);
    }
    s = fma(r[MODES], r[MODES], s);
    return sqrt(fmax(s, 0.0));
}

// rho_ij of the CQC rule (Der Kiureghian, equal damping) from the two circular frequencies
__device__ __forceinline__ double cqc_rho(const double wi, const double wj, const double zeta) {
    const double b = wj / wi, z2 = zeta * zeta, b1 = 1.0 + b, d = 1.0 - b * b;
    return 8.0 * z2 * b1 * (b * sqrt(b)) / (d * d + 4.0 * z2 * b * (b1 * b1));
}

// The spectrum of one direction at period Tk: linear between the table's points, constant outside them
__device__ __forceinline__ double spectrum_at(const double* __restrict__ T, const double* __restrict__ Sa, const int K,
                                              const double Tk) {
    if (!(Tk >= T[0])) return Sa[0];
    if (Tk >= T[K - 1]) return Sa[K - 1];
    int i = 0;
    while (i + 2 < K && T[i + 1] <= Tk) ++i;   // the largest i <= K - 2 with T[i] <= Tk
    const double t = (Tk - T[i]) / (T[i + 1] - T[i]);
    return fma(t, Sa[i + 1] - Sa[i], Sa[i]);
}

// Component `axis` of a direction, chosen among the three VALUES (a choice among the three places, inside a callable,
// is taken for an index at run time, and the directions then live in scratch)
__device__ __forceinline__ double component(const double (&d)[3], const int axis) {
    const double x = d[0], y = d[1], z = d[2];
    return axis == 0 ? x : axis == 1 ? y : z;
}

__global__ __launch_bounds__(256) void trs_rs_modal_kernel(
    const TrsBatch bt, const double* __restrict__ X_all, const double* __restrict__ lam_all,
    const double* __restrict__ Mf_all, const int* __restrict__ n_mass, const int p, const int G,
    const double* __restrict__ dirs, const int K, const double* __restrict__ T, const double* __restrict__ Sa,
    const double* __restrict__ zpa, const double zeta, const int rule, const int missing, double* __restrict__ gamma,
    double* __restrict__ sa_out, double* __restrict__ meff, double* __restrict__ mtot, double* __restrict__ base,
    double* __restrict__ q, double* __restrict__ rho, double* __restrict__ F_all) {
    constexpr int NSUM = DIRS * MODES + DIRS;   // Gamma of (g, k) at g * 8 + k, mtot of g behind them
    __shared__ double part[4][NSUM];          // the four waves' sums
    __shared__ double gam[DIRS][MODES];       // Gamma (0 for a mode that contributes nothing)
    __shared__ double mt[DIRS];               // mtot
    __shared__ double shear[DIRS][MODES];     // V_k = Gamma^2 sa
    __shared__ double om[MODES];              // omega, 0 for a mode that contributes nothing
    __shared__ double rh[MODES * MODES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int ld_f = bt.ld_f;
    const int n_modes = mode_count(n_mass, b, p);
    const double* Xb = X_all + (size_t)b * BLOCK * ld_f;
    const double* Mf = Mf_all + (size_t)b * ld_f;
    const double* lam = lam_all + (size_t)b * BLOCK;
    const unsigned use = part_mask(lam, n_modes);   // (a column of X outside it is never read into a result)

    double dir[DIRS][3];
#pragma unroll
    for (int g = 0; g < DIRS; ++g) {
#pragma unroll
        for (int a = 0; a < 3; ++a) dir[g][a] = g < G ? dirs[3 * g + a] : 0.0;
    }

    // ---- Gamma and mtot
    double acc[NSUM];
#pragma unroll
    for (int i = 0; i < NSUM; ++i) acc[i] = 0.0;
    each_dof(v, Mf, Xb, ld_f, use, tid, [&](const int row, const int axis, const double m, const double (&x)[MODES]) {
#pragma unroll
        for (int g = 0; g < DIRS; ++g) {
            const double io = component(dir[g], axis);
            const double mi = m * io;
            acc[DIRS * MODES + g] = fma(mi, io, acc[DIRS * MODES + g]);
#pragma unroll
            for (int k = 0; k < MODES; ++k) acc[g * MODES + k] = fma(mi, x[k], acc[g * MODES + k]);
        }
    });
    const double s = block_sums(acc, part, tid);
    if (tid < NSUM) {
        if (tid < DIRS * MODES)
            gam[tid / MODES][tid % MODES] = s;
        else
            mt[tid - DIRS * MODES] = s;
    }
    __syncthreads();

    // ---- per (direction, mode): the ordinate, the amplitude, the effective mass
    if (tid < DIRS * MODES) {
        const int g = tid / MODES, k = tid % MODES;
        const double l = lam[k];
        const bool good = takes_part(lam, k, n_modes), live = (g < G) & good;
        double ga = 0.0, s = 0.0, qv = 0.0, me = 0.0, w = 0.0;
        if (live) {
            ga = gam[g][k];
            w = sqrt(l);
            s = spectrum_at(T, Sa + (size_t)g * K, K, 6.283185307179586476925 / w);
            qv = ga * s / l;
            me = mt[g] > 0.0 ? ga * ga / mt[g] : 0.0;
        }
        gam[g][k] = ga;
        shear[g][k] = ga * ga * s;
        if (g == 0) om[k] = good ? sqrt(l) : 0.0;
        if ((g < G) & (k < p)) {
            const size_t o = ((size_t)b * G + g) * p + k;
            if (gamma != nullptr) gamma[o] = ga;
            if (sa_out != nullptr) sa_out[o] = s;
            if (meff != nullptr) meff[o] = me;
            q[o] = qv;
        }
    }
    __syncthreads();
    if (tid < MODES * MODES) {
        const int i = tid / MODES, j = tid % MODES;
        double r = 0.0;
        if ((om[i] > 0.0) & (om[j] > 0.0)) r = i == j ? 1.0 : rule == TRS_RS_CQC ? cqc_rho(om[i], om[j], zeta) : 0.0;
        rh[tid] = r;
        rho[(size_t)b * MODES * MODES + tid] = r;
    }
    __syncthreads();
    if (tid < G) {
        const int g = tid;
        double r[VEC], sum = 0.0;
#pragma unroll
        for (int k = 0; k < MODES; ++k) {
            r[k] = shear[g][k];
            sum = fma(gam[g][k], gam[g][k], sum);
        }
        r[MODES] = missing ? zpa[g] * (mt[g] - sum) : 0.0;
        if (mtot != nullptr) mtot[(size_t)b * G + g] = mt[g];
        if (base != nullptr) base[(size_t)b * G + g] = combine(rh, r, rule);
    }

    // ---- missing mass: f_g = zpa_g Mf (iota_g - sum_k Gamma_kg X_k) into column g, zeros everywhere else
    if (missing) {
        double* Fb = F_all + (size_t)b * BLOCK * ld_f;
        zero_columns(Fb, ld_f, 0, BLOCK, tid);
        __threadfence_block();
        __syncthreads();
        each_dof(v, Mf, Xb, ld_f, use, tid, [&](const int row, const int axis, const double m, const double (&x)[MODES]) {
#pragma unroll
            for (int g = 0; g < DIRS; ++g) {
                if (g >= G) continue;
                double rest = component(dir[g], axis);
#pragma unroll
                for (int k = 0; k < MODES; ++k) rest = fma(-gam[g][k], x[k], rest);
                Fb[(size_t)g * ld_f + row] = zpa[g] * (m * rest);
            }
        });
    }
}

// The signed modal member forces of direction g: slot k < p the mode's axial value scaled by q_gk, slot 8 the axial
// value of the missing-mass solution; zeros for a member that is not live.  ONE function (on member_axials' values: the
// axial value of every mode shape, no direction in it), so
// that N, modal_N and the reactions see the same values.
__device__ __forceinline__ void member_modal(const RsTables& t, const Member& mb, const double (&ax)[MODES],
                                             const int ndof_max, const int p, const int g, const bool missing,
                                             double (&r)[VEC]) {
#pragma unroll
    for (int k = 0; k < MODES; ++k) r[k] = t.q[g * MODES + k] * ax[k];
    r[MODES] = missing ? slot_axial(t.vec, mb, ndof_max, p + g) : 0.0;
}

__global__ __launch_bounds__(256) void trs_rs_combine_kernel(
    const TrsBatch bt, const double* __restrict__ X_all, const int* __restrict__ n_mass, const int p, const int G,
    const double* __restrict__ q_all, const double* __restrict__ rho_all, const int rule, const int missing_in,
    const double* __restrict__ F_all, double* __restrict__ u, double* __restrict__ R, double* __restrict__ N,
    double* __restrict__ modal_u, double* __restrict__ modal_R, double* __restrict__ modal_N) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max, ld_f = bt.ld_f, joints = v.joints, ndof_max = v.ndof_max;
    const int n_modes = mode_count(n_mass, b, p);
    const bool missing = missing_in != 0;
    const int nvec = p + (missing ? G : 0), V = p + 1;
    trs_lds::Carve lds(sh);
    const RsTables t = layout(lds, nJ_max, nM_max, nvec);
    const double* Xb = X_all + (size_t)b * BLOCK * ld_f;
    const double* Fb = missing ? F_all + (size_t)b * BLOCK * ld_f : nullptr;
    const bool want_R = (R != nullptr) | (modal_R != nullptr);

    // the modes that take part, from rho_kk != 0 (lam is not handed to this kernel): trs_rs_modal wrote 1 there for
    // exactly the modes of part_mask, 0 for the others - the same set
    unsigned live = 0;
#pragma unroll
    for (int k = 0; k < MODES; ++k)
        if ((k < n_modes) && rho_all[(size_t)b * MODES * MODES + k * (MODES + 1)] != 0.0) live |= 1u << k;

    // ---- stage: the mode shapes, then direction g's missing-mass solution
    stage_vectors(t.vec, v, Xb, ld_f, live, p, nvec, tid, [&](const int g, const int row) { return Fb[(size_t)g * ld_f + row]; });
    if (tid < MODES * MODES) t.rho[tid] = rho_all[(size_t)b * MODES * MODES + tid];
    if (tid < DIRS * MODES) {
        const int g = tid / MODES, k = tid % MODES;
        t.q[tid] = ((g < G) & in_mask(live, k)) ? q_all[((size_t)b * G + g) * p + k] : 0.0;
    }
    if (want_R) build_end_lists(t, v, tid);
    __syncthreads();

    // ---- members: N and modal_N, every member once
    if ((N != nullptr) | (modal_N != nullptr))
        for (int m = tid; m < nM_max; m += 256) {
            const Member mb = load_member(v, m);
            double ax[MODES];
            member_axials(t.vec, mb, ndof_max, p, ax);   // (once: the directions share them)
            for (int g = 0; g < G; ++g) {
                double r[VEC];
                member_modal(t, mb, ax, ndof_max, p, g, missing, r);
                const size_t row = (size_t)b * G + g;
                if (N != nullptr) N[row * nM_max + m] = combine(t.rho, r, rule);
                if (modal_N != nullptr) {
#pragma unroll
                    for (int k = 0; k < MODES; ++k)
                        if (k < p) modal_N[(row * V + k) * nM_max + m] = r[k];
                    modal_N[(row * V + p) * nM_max + m] = r[MODES];
                }
            }
        }

    // ---- joints: u and modal_u; R and modal_R from the joint's member-end list, member-id order
    if ((u != nullptr) | (modal_u != nullptr) | want_R)
        for (int j = tid; j < nJ_max; j += 256) {
            const bool own = j < joints;
            const int o = v.place(j);
            bool held[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) held[a] = own & v.held(j, a);
            for (int g = 0; g < G; ++g) {
                const size_t row = (size_t)b * G + g;
                if ((u != nullptr) | (modal_u != nullptr)) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        double r[VEC];
#pragma unroll
                        for (int k = 0; k < MODES; ++k)
                            r[k] = (own & (k < p)) ? t.q[g * MODES + k] * t.vec[(size_t)k * ndof_max + 3 * j + a] : 0.0;
                        r[MODES] = (own & missing) ? t.vec[(size_t)(p + g) * ndof_max + 3 * j + a] : 0.0;
                        if (u != nullptr) u[(row * nJ_max + o) * 3 + a] = combine(t.rho, r, rule);
                        if (modal_u != nullptr) {
#pragma unroll
                            for (int k = 0; k < MODES; ++k)
                                if (k < p) modal_u[((row * V + k) * nJ_max + o) * 3 + a] = r[k];
                            modal_u[((row * V + p) * nJ_max + o) * 3 + a] = r[MODES];
                        }
                    }
                }
                if (want_R) {
                    double acc[VEC][3];
                    const EndList l = end_list(t, j, held[0] | held[1] | held[2], acc);
                    for (int i = 0; i < l.deg; ++i) {
                        const Member mb = load_member(v, l.ends[i] >> 1);
                        double ax[MODES], r[VEC];
                        member_axials(t.vec, mb, ndof_max, p, ax);
                        member_modal(t, mb, ax, ndof_max, p, g, missing, r);
                        add_end_forces(acc, mb, r, l.ends[i] & 1);
                    }
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        double r[VEC];
#pragma unroll
                        for (int k = 0; k < VEC; ++k) r[k] = held[a] ? acc[k][a] : 0.0;
                        if (R != nullptr) R[(row * nJ_max + o) * 3 + a] = combine(t.rho, r, rule);
                        if (modal_R != nullptr) {
#pragma unroll
                            for (int k = 0; k < MODES; ++k)
                                if (k < p) modal_R[((row * V + k) * nJ_max + o) * 3 + a] = r[k];
                            modal_R[((row * V + p) * nJ_max + o) * 3 + a] = r[MODES];
                        }
                    }
                }
            }
        }
}

bool rs_args_ok(int p, int G, int rule) {
    return p >= 1 && p <= TRS_RS_MAX_MODES && G >= 1 && G <= TRS_RS_MAX_DIRS && rule >= TRS_RS_SRSS && rule <= TRS_RS_ABS;
}

int rs_combine_launch(int B, const TrsBatch& bt, const double* X, const int* n_mass, int p, int G, const double* q,
                      const double* rho, int rule, int missing, const double* F, double* u, double* R, double* N,
                      double* modal_u, double* modal_R, double* modal_N, hipStream_t stream) {
    if (B <= 0) return 0;
    if (!rs_args_ok(p, G, rule) || !trs_rs_fits(bt.nJ_max, bt.nM_max, p) || bt.ld_f < 1 || X == nullptr ||
        n_mass == nullptr || q == nullptr || rho == nullptr || (missing && F == nullptr))
        return (int)hipErrorInvalidValue;
    if (u == nullptr && R == nullptr && N == nullptr && modal_u == nullptr && modal_R == nullptr && modal_N == nullptr)
        return 0;
    trs_lds::raise_lds_once<trs_rs_combine_kernel>();
    hipLaunchKernelGGL(trs_rs_combine_kernel, dim3(B), dim3(256), rs_lds(bt.nJ_max, bt.nM_max, p + (missing ? G : 0)),
                       stream, bt, X, n_mass, p, G, q, rho, rule, missing, F, u, R, N, modal_u, modal_R, modal_N);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_rs_abi_version(void) { return TRS_RS_ABI_VERSION; }

int trs_rs_fits(int nJ_max, int nM_max, int p) {
    return nJ_max >= 0 && nM_max >= 0 && p >= 1 && p <= TRS_RS_MAX_MODES &&
           rs_lds(nJ_max, nM_max, p + TRS_RS_MAX_DIRS) <= TRS_LDS_BYTES;
}

int trs_rs_modal(int B, int nJ_max, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const double* X,
                 int ld_f, const double* lam, const double* Mf, const int32_t* n_mass, int p, int G, const double* dirs,
                 int K, const double* T, const double* Sa, const double* zpa, double zeta, int rule, int missing_mass,
                 double* gamma, double* sa, double* meff, double* mtot, double* base, double* q, double* rho, double* F,
                 void* stream) {
    if (B <= 0) return 0;
    if (!rs_args_ok(p, G, rule) || K < 2 || K > TRS_RS_MAX_TABLE || nJ_max < 0 || ld_f < 1 || X == nullptr ||
        lam == nullptr || Mf == nullptr || n_mass == nullptr || dirs == nullptr || T == nullptr || Sa == nullptr ||
        q == nullptr || rho == nullptr || (rule == TRS_RS_CQC && !(zeta > 0.0)) ||
        (missing_mass && (F == nullptr || zpa == nullptr)))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(trs_rs_modal_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream,
                       trs_batch_dofs(nJ_max, free_index, n_free, nJ, nullptr, ld_f), X, lam, Mf, n_mass, p, G, dirs, K, T,
                       Sa, zpa, zeta, rule, missing_mass, gamma, sa, meff, mtot, base, q, rho, F);
    return (int)hipGetLastError();
}

int trs_rs_combine(int B, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E, const double* A,
                   const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM,
                   const int32_t* joint_out, const double* X, int ld_f, const int32_t* n_mass, int p, int G,
                   const double* q, const double* rho, int rule, int missing_mass, const double* F, double* u, double* R,
                   double* N, double* modal_u, double* modal_R, double* modal_N, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, n_free, nJ, nM,
                                  joint_out, ld_f);
    return rs_combine_launch(B, bt, X, n_mass, p, G, q, rho, rule, missing_mass, F, u, R, N, modal_u, modal_R, modal_N,
                             (hipStream_t)stream);
}

int trs_rs_combine_tab(int B, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16, const uint8_t* type_idx,
                       const double* types, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                       const int32_t* nM, const int32_t* joint_out, const double* X, int ld_f, const int32_t* n_mass, int p,
                       int G, const double* q, const double* rho, int rule, int missing_mass, const double* F, double* u,
                       double* R, double* N, double* modal_u, double* modal_R, double* modal_N, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free, nJ,
                                  nM, joint_out, ld_f);
    return rs_combine_launch(B, bt, X, n_mass, p, G, q, rho, rule, missing_mass, F, u, R, N, modal_u, modal_R, modal_N,
                             (hipStream_t)stream);
}

}  // extern "C"
