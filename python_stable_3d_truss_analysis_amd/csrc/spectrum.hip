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
// missing-mass solutions behind them), as trs_mg_grad stages phi; then
//   members   one thread per member, visited once: geometry and E A in registers, the axial value of every mode formed
//             once and scaled by q per direction - up to nine modal values in registers, compile-time indexed
//   joints    one thread per joint: u per direction and component; for a joint with a held DOF the thread walks the
//             joint's member-end list in member-id order (trs_rec::build_end_lists) for R
// No floating-point atomic, every sum in one fixed order.  member_axials / member_modal and combine are the ONE function
// each that the member pass, the reaction pass and the base shear share.  A column of X whose lam contributes nothing is
// read by neither kernel.
#include "../../include/trs_spectrum.h"
#include "../../include/trs_modes.h"
#include "trs_common.h"
#include "trs_lds.h"

namespace {

using namespace trs_rec;

static_assert(TRS_RS_BLOCK == TRS_MODES_BLOCK, "the block of trs_spectrum.h is the one of trs_modes.h");
static_assert(TRS_RS_MAX_VEC == TRS_RS_MAX_MODES + 1, "the modes and the missing-mass slot");
constexpr int MODES = TRS_RS_MAX_MODES, DIRS = TRS_RS_MAX_DIRS, VEC = TRS_RS_MAX_VEC;

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

__global__ __launch_bounds__(256) void trs_rs_modal_kernel(
    const TrsBatch bt, const double* __restrict__ X_all, const double* __restrict__ lam_all,
    const double* __restrict__ Mf_all, const int* __restrict__ n_mass, const int p, const int G,
    const double* __restrict__ dirs, const int K, const double* __restrict__ T, const double* __restrict__ Sa,
    const double* __restrict__ zpa, const double zeta, const int rule, const int missing, double* __restrict__ gamma,
    double* __restrict__ sa_out, double* __restrict__ meff, double* __restrict__ mtot, double* __restrict__ base,
    double* __restrict__ q, double* __restrict__ rho, double* __restrict__ F_all) {
    constexpr int NSUM = DIRS * MODES + DIRS;
    __shared__ double part[4][NSUM];          // the four waves' sums
    __shared__ double gam[DIRS][MODES];       // Gamma (0 for a mode that contributes nothing)
    __shared__ double mt[DIRS];               // mtot
    __shared__ double shear[DIRS][MODES];     // V_k = Gamma^2 sa
    __shared__ double om[MODES];              // omega, 0 for a mode that contributes nothing
    __shared__ double rh[MODES * MODES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int ld_f = bt.ld_f, ndof = v.ndof;
    const int n_modes = min(p, max(n_mass[b], 0));
    const double* Xb = X_all + (size_t)b * TRS_RS_BLOCK * ld_f;
    const double* Mf = Mf_all + (size_t)b * ld_f;
    const double* lam = lam_all + (size_t)b * TRS_RS_BLOCK;

    double dir[DIRS][3];
#pragma unroll
    for (int g = 0; g < DIRS; ++g) {
#pragma unroll
        for (int a = 0; a < 3; ++a) dir[g][a] = g < G ? dirs[3 * g + a] : 0.0;
    }

    // the modes that contribute: a column of X whose lam is not positive and finite is never read into a result
    bool use[MODES];
#pragma unroll
    for (int k = 0; k < MODES; ++k) {
        const double l = k < n_modes ? lam[k] : 0.0;
        use[k] = (l > 0.0) & (l < INFINITY);
    }

    // ---- Gamma and mtot: this thread's DOFs in ascending order
    double acc[DIRS][MODES], am[DIRS];
#pragma unroll
    for (int g = 0; g < DIRS; ++g) {
        am[g] = 0.0;
#pragma unroll
        for (int k = 0; k < MODES; ++k) acc[g][k] = 0.0;
    }
    for (int d = tid; d < ndof; d += 256) {
        const int row = v.row_of(d), axis = d % 3;
        if (row < 0) continue;
        const double m = Mf[row];
        double x[MODES];
#pragma unroll
        for (int k = 0; k < MODES; ++k) x[k] = use[k] ? Xb[(size_t)k * ld_f + row] : 0.0;
#pragma unroll
        for (int g = 0; g < DIRS; ++g) {
            const double io = axis == 0 ? dir[g][0] : axis == 1 ? dir[g][1] : dir[g][2];
            const double mi = m * io;
            am[g] = fma(mi, io, am[g]);
#pragma unroll
            for (int k = 0; k < MODES; ++k) acc[g][k] = fma(mi, x[k], acc[g][k]);
        }
    }
    // the wave's 64 partials by the butterfly, then the four waves in order
    auto fold = [](double v) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        return v;
    };
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int g = 0; g < DIRS; ++g) {
#pragma unroll
        for (int k = 0; k < MODES; ++k) {
            const double s = fold(acc[g][k]);
            if (lane == 0) part[wave][g * MODES + k] = s;
        }
        const double s = fold(am[g]);
        if (lane == 0) part[wave][DIRS * MODES + g] = s;
    }
    __syncthreads();
    if (tid < NSUM) {
        const double s = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
        if (tid < DIRS * MODES)
            gam[tid / MODES][tid % MODES] = s;
        else
            mt[tid - DIRS * MODES] = s;
    }
    __syncthreads();

    // ---- per (direction, mode): the ordinate, the amplitude, the effective mass
    if (tid < DIRS * MODES) {
        const int g = tid / MODES, k = tid % MODES;
        const double l = k < n_modes ? lam[k] : 0.0;
        const bool good = (l > 0.0) & (l < INFINITY);   // the mode contributes (use[k])
        const bool live = (g < G) & good;
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
        double* Fb = F_all + (size_t)b * TRS_RS_BLOCK * ld_f;
        for (int x = tid; x < TRS_RS_BLOCK * ld_f; x += 256) Fb[x] = 0.0;
        __threadfence_block();
        __syncthreads();   // (the zeros of another thread lie under this thread's entries)
        for (int d = tid; d < ndof; d += 256) {
            const int row = v.row_of(d), axis = d % 3;
            if (row < 0) continue;
            const double m = Mf[row];
            double x[MODES];
#pragma unroll
            for (int k = 0; k < MODES; ++k) x[k] = use[k] ? Xb[(size_t)k * ld_f + row] : 0.0;
#pragma unroll
            for (int g = 0; g < DIRS; ++g) {
                if (g >= G) continue;
                double rest = axis == 0 ? dir[g][0] : axis == 1 ? dir[g][1] : dir[g][2];
#pragma unroll
                for (int k = 0; k < MODES; ++k) rest = fma(-gam[g][k], x[k], rest);
                Fb[(size_t)g * ld_f + row] = zpa[g] * (m * rest);
            }
        }
    }
}

// One member as the passes of the combine kernel see it
struct RsMember {
    MemberGeom g;
    double ea;
    int2 c;       // end joints, clamped
    bool live;    // inside the truss and of positive length
};
__device__ __forceinline__ RsMember load_member(const TrussView& v, const int m) {
    RsMember r;
    r.live = m < v.members;
    r.c = int2{0, 0};
    r.ea = 0.0;
    r.g.len = 0.0;
    r.g.c[0] = r.g.c[1] = r.g.c[2] = 0.0;
    if (r.live) {
        // an end outside the truss is on no end list: the member then gives zeros to N as it does to R
        const TrussView::Ends e = v.ends(m);
        r.c = e.c;
        r.g = member_geom(v.X, e.c.x, e.c.y);
        r.ea = v.mem.EA(v.mbase + m);
        r.live = e.inside & (r.g.len > 0.0);
    }
    return r;
}

// The axial value of every mode shape in a member (no direction in it: q carries that); zeros for a member that is not live
__device__ __forceinline__ void member_axials(const RsTables& t, const RsMember& mb, const int ndof_max, const int p,
                                              double (&ax)[MODES]) {
#pragma unroll
    for (int k = 0; k < MODES; ++k) {
        ax[k] = 0.0;
        if (mb.live & (k < p)) ax[k] = member_axial(mb.g, mb.ea, t.vec + (size_t)k * ndof_max, mb.c.x, mb.c.y);
    }
}

// The signed modal member forces of direction g: slot k < p the mode's axial value scaled by q_gk, slot 8 the axial
// value of the missing-mass solution; zeros for a member that is not live.  ONE function (on member_axials' values), so
// that N, modal_N and the reactions see the same values.
__device__ __forceinline__ void member_modal(const RsTables& t, const RsMember& mb, const double (&ax)[MODES],
                                             const int ndof_max, const int p, const int g, const bool missing,
                                             double (&r)[VEC]) {
#pragma unroll
    for (int k = 0; k < MODES; ++k) r[k] = t.q[g * MODES + k] * ax[k];
    r[MODES] = 0.0;
    if (mb.live & missing) r[MODES] = member_axial(mb.g, mb.ea, t.vec + (size_t)(p + g) * ndof_max, mb.c.x, mb.c.y);
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
    const int n_modes = min(p, max(n_mass[b], 0));
    const bool missing = missing_in != 0;
    const int nvec = p + (missing ? G : 0), V = p + 1;
    trs_lds::Carve lds(sh);
    const RsTables t = layout(lds, nJ_max, nM_max, nvec);
    const double* Xb = X_all + (size_t)b * TRS_RS_BLOCK * ld_f;
    const double* Fb = missing ? F_all + (size_t)b * TRS_RS_BLOCK * ld_f : nullptr;
    const bool want_R = (R != nullptr) | (modal_R != nullptr);

    // the modes that contribute (rho_kk != 0): a column of X whose lam is not positive and finite is never read
    unsigned live = 0;
#pragma unroll
    for (int k = 0; k < MODES; ++k)
        if ((k < n_modes) && rho_all[(size_t)b * MODES * MODES + k * (MODES + 1)] != 0.0) live |= 1u << k;

    // ---- stage: every response vector in joint layout, zero at held DOFs and past the truss's own joints
    for (int x = tid; x < nvec * ndof_max; x += 256) {
        const int k = x / ndof_max, d = x - k * ndof_max;
        const int row = v.row_of(d);
        double val = 0.0;
        if (row >= 0) {
            if (k >= p)
                val = Fb[(size_t)(k - p) * ld_f + row];
            else if ((live >> k) & 1u)
                val = Xb[(size_t)k * ld_f + row];
        }
        t.vec[x] = val;
    }
    if (tid < MODES * MODES) t.rho[tid] = rho_all[(size_t)b * MODES * MODES + tid];
    if (tid < DIRS * MODES) {
        const int g = tid / MODES, k = tid % MODES;
        t.q[tid] = ((g < G) & (((live >> k) & 1u) != 0)) ? q_all[((size_t)b * G + g) * p + k] : 0.0;
    }
    if (want_R) build_end_lists(t, v, tid);
    __syncthreads();

    // ---- members: N and modal_N, every member once
    if ((N != nullptr) | (modal_N != nullptr))
        for (int m = tid; m < nM_max; m += 256) {
            const RsMember mb = load_member(v, m);
            double ax[MODES];
            member_axials(t, mb, ndof_max, p, ax);   // (once: the directions share them)
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
            const bool any_held = held[0] | held[1] | held[2];
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
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
                    const int* list = t.ends + (any_held ? t.start[j] : 0);
                    const int deg = any_held ? t.cnt[j] : 0;
                    for (int i = 0; i < deg; ++i) {
                        const int m = list[i] >> 1, end = list[i] & 1;
                        const RsMember mb = load_member(v, m);
                        double ax[MODES], r[VEC];
                        member_axials(t, mb, ndof_max, p, ax);
                        member_modal(t, mb, ax, ndof_max, p, g, missing, r);
                        if (mb.live) {
#pragma unroll
                            for (int k = 0; k < VEC; ++k) add_end_force(acc[k], mb.g.c, r[k], end);
                        }
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
