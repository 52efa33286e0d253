// Harmonic response over a frequency sweep from the converged mode block (include/trs_harmonic.h): the steady-state
// amplitude of every displacement, member force and support reaction under M u'' + C u' + K u = Re(f e^(i W t)) by mode
// superposition with the block X that trs_modes_step left resident and - for the static correction of the truncated
// modes - one more substitution against the resident factor (trs_potrs_cases, unchanged, between the two kernels).
//
//   trs_hr_modal   X, lam, Mf, the reduced load patterns and the ground accelerations -> the modal loads g [B][L][p]
//                  and, with the residual, the residual loads in F [B][16][ld_f]
//   trs_hr_sweep   X, lam, g (and the solved F), omega [S] -> the envelopes u_amp, R_amp [B][L][nJ_max][3],
//                  N_amp [B][L][nM_max] with the index that attains each, and (Re, Im) of the monitored joints and
//                  members at every frequency
//
// Both are one work-group of 256 threads per (truss, case).  The walk over the DOFs and its reduction, the stage of the
// p mode shapes and the case's u_res in LDS in joint layout, the member and the end forces of a joint are the ones of
// spectrum.hip: trs_modal.h.  The hot loop of trs_hr_sweep is arithmetic: an item (a member, a joint's three components)
// forms its p + 1 real coefficients ONCE, in registers, and then runs the frequencies against the table
// c_lk(W_s) = g_lk H_k(W_s) of one chunk of 64 frequencies, built cooperatively in LDS and read by all lanes at the same
// address (a broadcast): 2 p + 1 fused multiply-adds per item and frequency, and a square root only where |y|^2 sets a
// new peak.  The loop over an item group (512 members, 256 joints) and the loop over the chunks inside it have trip
// counts that are uniform over the work-group; the barriers around the table sit in those two loops only.
// No floating-point atomic, every sum in one fixed order.  sweep_chunk is the ONE function that turns coefficients and
// table into (Re, Im) per frequency: the three passes and the monitors call it, so a monitored value and the envelope
// at the same index are the same number.
#include "trs_modal.h"

namespace {

using namespace trs_rec;
using namespace trs_modal;

constexpr int CHUNK = TRS_HR_CHUNK;
static_assert(MODES == 8 && (CHUNK * MODES) % 256 == 0, "a thread builds the table entries of ONE mode: tid % 8");

// LDS of the sweep kernel
struct HrTables : EndLists {   // (the member-end lists of every joint of the truss: trs_recover.h)
    double* tab;               // [64][8][2]         (Re, Im) of c_lk(W_s) of the chunk, 0 where there is none; first: it
                               //                    is read as double2, and the head of the LDS is aligned to 16
    double* g;                 // [8]                the case's modal loads, 0 where there is none
    double* vec;               // [p + 1][3 nJ_max]  the response vectors, joint layout: modes 0 .. p - 1, then u_res
};

template <class Arena>
__host__ __device__ inline HrTables layout(Arena& a, int nJ_max, int nM_max, int p) {
    HrTables t;
    t.tab = a.template take<double>(CHUNK * MODES * 2);
    t.g = a.template take<double>(MODES);
    t.vec = a.template take<double>((size_t)(p + 1) * 3 * nJ_max);
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    return t;
}

size_t hr_lds(int nJ_max, int nM_max, int p) {
    return trs_lds::count([&](auto& a) { layout(a, nJ_max, nM_max, p); });
}

__global__ __launch_bounds__(256) void trs_hr_modal_kernel(
    const TrsBatch bt, const int L, const double* __restrict__ X_all, const double* __restrict__ lam_all,
    const double* __restrict__ Mf_all, const int* __restrict__ n_mass, const int p, const double* __restrict__ Pr_all,
    const double* __restrict__ ag_all, const int residual, double* __restrict__ g_all, double* __restrict__ F_all) {
    __shared__ double part[4][MODES];   // the four waves' sums
    __shared__ double gl[MODES];        // g (0 for a mode that contributes nothing)
    const int b = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int ld_f = bt.ld_f;
    const int n_modes = mode_count(n_mass, b, p);
    const double* Xb = X_all + (size_t)b * BLOCK * ld_f;
    const double* Mf = Mf_all + (size_t)b * ld_f;
    const double* lam = lam_all + (size_t)b * BLOCK;
    const unsigned use = part_mask(lam, n_modes);   // (a column of X outside it is never read into a result)
    const double* Pr = Pr_all != nullptr ? Pr_all + ((size_t)b * L + l) * ld_f : nullptr;
    double acc_g[3] = {0.0, 0.0, 0.0};   // the ground acceleration of the case
    if (ag_all != nullptr) {
#pragma unroll
        for (int a = 0; a < 3; ++a) acc_g[a] = ag_all[((size_t)b * L + l) * 3 + a];
    }

    // f of DOF d at reduced row `row`: P - Mf iota(ag)
    auto load_of = [&](const int row, const int axis, const double m) {
        const double a = axis == 0 ? acc_g[0] : axis == 1 ? acc_g[1] : acc_g[2];
        return fma(-m, a, Pr != nullptr ? Pr[row] : 0.0);
    };

    // ---- g
    double acc[MODES];
#pragma unroll
    for (int k = 0; k < MODES; ++k) acc[k] = 0.0;
    each_dof(v, Mf, Xb, ld_f, use, tid, [&](const int row, const int axis, const double m, const double (&x)[MODES]) {
        const double f = load_of(row, axis, m);
#pragma unroll
        for (int k = 0; k < MODES; ++k) acc[k] = fma(f, x[k], acc[k]);
    });
    const double s = block_sums(acc, part, tid);
    if (tid < MODES) {
        const double gv = takes_part(lam, tid, n_modes) ? s : 0.0;
        gl[tid] = gv;
        if (tid < p) g_all[((size_t)b * L + l) * p + tid] = gv;
    }
    __syncthreads();

    // ---- the residual load: f - Mf (sum_k g_k X_k) into column l; the work-group of case 0 zeroes the columns L .. 15
    if (residual) {
        double* Fb = F_all + (size_t)b * BLOCK * ld_f;
        double* col = Fb + (size_t)l * ld_f;
        zero_columns(Fb, ld_f, l, l + 1, tid);
        if (l == 0) zero_columns(Fb, ld_f, L, BLOCK, tid);
        __threadfence_block();
        __syncthreads();
        each_dof(v, Mf, Xb, ld_f, use, tid, [&](const int row, const int axis, const double m, const double (&x)[MODES]) {
            double rest = load_of(row, axis, m);
#pragma unroll
            for (int k = 0; k < MODES; ++k) rest = fma(-gl[k], m * x[k], rest);
            col[row] = rest;
        });
    }
}

// The p + 1 real coefficients of a member force: the axial value of every mode shape, and of u_res in slot 8; zeros for
// a member that is not live and for the slots p .. 7.  ONE function, so that N, the reactions and the monitors see the
// same values.
__device__ __forceinline__ void member_coefficients(const HrTables& t, const Member& mb, const int ndof_max,
                                                    const int p, double (&y)[VEC]) {
    member_axials(t.vec, mb, ndof_max, p, y);
    y[MODES] = slot_axial(t.vec, mb, ndof_max, p);
}

// The coefficients of joint j's three displacement components (zeros for a joint that is not `own`)
__device__ __forceinline__ void joint_coefficients(const HrTables& t, const int j, const bool own, const int ndof_max,
                                                   const int p, double (&y)[3][VEC]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int k = 0; k < MODES; ++k) y[a][k] = (own & (k < p)) ? t.vec[(size_t)k * ndof_max + 3 * j + a] : 0.0;
        y[a][MODES] = own ? t.vec[(size_t)p * ndof_max + 3 * j + a] : 0.0;
    }
}

// |y|^2 of a response, the one form every amplitude is the root of
__device__ __forceinline__ double modulus2(const double re, const double im) { return fma(re, re, im * im); }

// (Re, Im) of N items at the `count` frequencies of the table, handed to `sink(i, s, re, im)`: Re from y_res and Im
// from 0, by fused multiply-adds over the modes in ascending order.  The slots p .. 7 hold zeros on both sides and are
// skipped.  Four frequencies are in flight at a time: the chains of one frequency are eight dependent operations long,
// and a work-group that fills half a CU's LDS leaves a SIMD two waves to hide them behind (EXPERIMENTS R27).
template <int N, class Sink>
__device__ __forceinline__ void sweep_chunk(const double (&y)[N][VEC], const double* tab, const int count, const int s0,
                                            const int p, Sink& sink) {
    const double2* row = reinterpret_cast<const double2*>(tab);
#pragma unroll 4
    for (int s = 0; s < count; ++s, row += MODES) {
        double re[N], im[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            re[i] = y[i][MODES];
            im[i] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < MODES; ++k) {
            if (k < p) {
                const double2 c = row[k];   // (every lane the same address: a broadcast)
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    re[i] = fma(y[i][k], c.x, re[i]);
                    im[i] = fma(y[i][k], c.y, im[i]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i) sink(i, s0 + s, re[i], im[i]);
    }
}

// What a pass needs to run the S frequencies: where the table lies and this thread's share of building it - the
// entries of mode tid % 8 (lam, 2 zeta_k w_k and g of that mode; live: the mode takes part)
struct HrSweep {
    double* tab;
    const double* omega;
    int S, p, tid;
    double lam, tzw, g;
    bool live;
};

// The S frequencies of the thread's items, chunk by chunk: the table of the chunk is built by the whole work-group (two
// entries per thread), then every `active` thread runs its items against it.  Called by ALL threads of the work-group;
// S is uniform, so are the barriers.
template <int N, class Sink>
__device__ __forceinline__ void sweep_all(const HrSweep& c, const double (&y)[N][VEC], const bool active, Sink& sink) {
    double2* tab = reinterpret_cast<double2*>(c.tab);
    for (int s0 = 0; s0 < c.S; s0 += CHUNK) {
        __syncthreads();   // (the readers of the previous table are done)
        for (int e = c.tid; e < CHUNK * MODES; e += 256) {
            const int s = s0 + e / MODES;
            double2 val = double2{0.0, 0.0};
            if (c.live & (s < c.S)) {
                const double W = c.omega[s];
                const double dr = fma(-W, W, c.lam), di = c.tzw * W;
                const double n2 = fma(dr, dr, di * di);
                val = double2{c.g * (dr / n2), c.g * (-di / n2)};
            }
            tab[e] = val;
        }
        __syncthreads();
        if (active) sweep_chunk<N>(y, c.tab, min(CHUNK, c.S - s0), s0, c.p, sink);
    }
}

// The envelope of N items: index 0 initialises, a later index replaces only when its amplitude sqrt(|y|^2) is strictly
// greater.  The root is monotone, so it is taken only where |y|^2 exceeds the largest seen so far (top2): anywhere else
// the amplitude cannot exceed `best`.  Two |y|^2 one rounding apart can share a root; then top2 moves on and the first
// index stays, as the header has it.
template <int N>
struct Envelope {
    double best[N], top2[N];
    int at[N];
    __device__ __forceinline__ Envelope() {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            best[i] = top2[i] = -1.0;
            at[i] = 0;
        }
    }
    __device__ __forceinline__ void operator()(const int i, const int s, const double re, const double im) {
        const double a2 = modulus2(re, im);
        if (a2 > top2[i]) {
            top2[i] = a2;
            const double amp = sqrt(a2);
            if (amp > best[i]) {
                best[i] = amp;
                at[i] = s;
            }
        }
    }
};

// (Re, Im) of N items of monitor `idx` of `count` at every frequency: out [S][count][N][2]
template <int N>
struct Monitor {
    double* out;
    int count, idx;
    __device__ __forceinline__ void operator()(const int i, const int s, const double re, const double im) {
        double2* at = reinterpret_cast<double2*>(out) + ((size_t)s * count + idx) * N + i;
        *at = double2{re, im};
    }
};

__global__ __launch_bounds__(256) void trs_hr_sweep_kernel(
    const TrsBatch bt, const int L, const double* __restrict__ X_all, const double* __restrict__ lam_all,
    const int* __restrict__ n_mass, const int p, const double* __restrict__ g_all, const double* __restrict__ F_all,
    const int S, const double* __restrict__ omega, const double zeta, const double damp_mass, const double damp_stiff,
    double* __restrict__ u_amp, int* __restrict__ u_at, double* __restrict__ R_amp, int* __restrict__ R_at,
    double* __restrict__ N_amp, int* __restrict__ N_at, const int* __restrict__ mon_joint, const int Pj,
    const int* __restrict__ mon_member, const int Pm, double* __restrict__ frf_u, double* __restrict__ frf_N) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max, ld_f = bt.ld_f, joints = v.joints, ndof_max = v.ndof_max;
    const int n_modes = mode_count(n_mass, b, p);
    trs_lds::Carve lds(sh);
    const HrTables t = layout(lds, nJ_max, nM_max, p);
    const double* Xb = X_all + (size_t)b * BLOCK * ld_f;
    const double* lam = lam_all + (size_t)b * BLOCK;
    const double* ures = F_all != nullptr ? F_all + ((size_t)b * BLOCK + l) * ld_f : nullptr;
    const size_t row = (size_t)b * L + l;
    const bool want_u = (u_amp != nullptr) | (u_at != nullptr), want_R = (R_amp != nullptr) | (R_at != nullptr);
    const bool want_N = (N_amp != nullptr) | (N_at != nullptr);

    const unsigned live = part_mask(lam, n_modes);   // (a column of X outside it is never read)

    // ---- stage: the mode shapes, then the case's u_res
    stage_vectors(t.vec, v, Xb, ld_f, live, p, p + 1, tid, [&](int, const int r) { return ures != nullptr ? ures[r] : 0.0; });
    if (tid < MODES) t.g[tid] = in_mask(live, tid) ? g_all[row * p + tid] : 0.0;
    if (want_R) build_end_lists(t, v, tid);
    __syncthreads();

    // this thread's share of every table: mode tid % 8
    HrSweep sw;
    sw.tab = t.tab;
    sw.omega = omega;
    sw.S = S;
    sw.p = p;
    sw.tid = tid;
    {
        const int k = tid % MODES;
        sw.live = in_mask(live, k);
        sw.lam = sw.live ? lam[k] : 1.0;
        const double w = sqrt(sw.lam);
        const double zk = zeta + damp_mass / (2.0 * w) + damp_stiff * w / 2.0;
        sw.tzw = (2.0 * zk) * w;
        sw.g = t.g[k];
    }

    // ---- members: N_amp and N_at, two members per thread (m and m + 256: one read of the table serves both, and their
    // chains are independent)
    if (want_N)
        for (int m0 = 0; m0 < nM_max; m0 += 512) {
            double y[2][VEC];
            bool live[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = m0 + 256 * i + tid;
                const Member mb = load_member(v, m < nM_max ? m : -1);
                member_coefficients(t, mb, ndof_max, p, y[i]);
                live[i] = mb.live;
            }
            Envelope<2> env;
            sweep_all<2>(sw, y, live[0] | live[1], env);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = m0 + 256 * i + tid;
                if (m < nM_max) {
                    if (N_amp != nullptr) N_amp[row * nM_max + m] = live[i] ? env.best[i] : 0.0;
                    if (N_at != nullptr) N_at[row * nM_max + m] = live[i] ? env.at[i] : 0;
                }
            }
        }

    // ---- joints: u_amp and u_at, one thread per joint and its three components
    if (want_u)
        for (int j0 = 0; j0 < nJ_max; j0 += 256) {
            const int j = j0 + tid;
            const bool mine = j < nJ_max, own = j < joints;
            double y[3][VEC];
            joint_coefficients(t, own ? j : 0, own, ndof_max, p, y);
            Envelope<3> env;
            sweep_all<3>(sw, y, own, env);
            if (mine) {
                const int o = v.place(j);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const bool free_dof = own && !v.held(j, a);
                    if (u_amp != nullptr) u_amp[(row * nJ_max + o) * 3 + a] = free_dof ? env.best[a] : 0.0;
                    if (u_at != nullptr) u_at[(row * nJ_max + o) * 3 + a] = free_dof ? env.at[a] : 0;
                }
            }
        }

    // ---- joints with a held DOF: R_amp and R_at from the joint's member-end list, member-id order
    if (want_R)
        for (int j0 = 0; j0 < nJ_max; j0 += 256) {
            const int j = j0 + tid;
            const bool mine = j < nJ_max, own = j < joints;
            bool held[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) held[a] = own && v.held(j, a);
            double acc[VEC][3], y[3][VEC];
            const bool any_held = held[0] | held[1] | held[2];
            const EndList el = end_list(t, j, any_held, acc);
            for (int i = 0; i < el.deg; ++i) {
                const Member mb = load_member(v, el.ends[i] >> 1);
                double r[VEC];
                member_coefficients(t, mb, ndof_max, p, r);
                add_end_forces(acc, mb, r, el.ends[i] & 1);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) y[a][k] = held[a] ? acc[k][a] : 0.0;
            }
            Envelope<3> env;
            sweep_all<3>(sw, y, any_held, env);
            if (mine) {
                const int o = v.place(j);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (R_amp != nullptr) R_amp[(row * nJ_max + o) * 3 + a] = held[a] ? env.best[a] : 0.0;
                    if (R_at != nullptr) R_at[(row * nJ_max + o) * 3 + a] = held[a] ? env.at[a] : 0;
                }
            }
        }

    // ---- the monitors: (Re, Im) at every frequency, by the same function on the same coefficients
    if (frf_u != nullptr)
        for (int i0 = 0; i0 < Pj; i0 += 256) {
            const int i = i0 + tid;
            const bool mine = i < Pj;
            const int j = mine ? mon_joint[(size_t)b * Pj + i] : -1;
            const bool own = v.in_truss(j);
            double y[3][VEC];
            joint_coefficients(t, own ? j : 0, own, ndof_max, p, y);
            Monitor<3> mon{frf_u + row * S * Pj * 6, Pj, i};
            sweep_all<3>(sw, y, mine, mon);
        }
    if (frf_N != nullptr)
        for (int i0 = 0; i0 < Pm; i0 += 256) {
            const int i = i0 + tid;
            const bool mine = i < Pm;
            const Member mb = load_member(v, mine ? mon_member[(size_t)b * Pm + i] : -1);
            double y[1][VEC];
            member_coefficients(t, mb, ndof_max, p, y[0]);
            Monitor<1> mon{frf_N + row * S * Pm * 2, Pm, i};
            sweep_all<1>(sw, y, mine, mon);
        }
}

bool hr_args_ok(int L, int p) { return p >= 1 && p <= TRS_HR_MAX_MODES && L >= 1 && L <= TRS_HR_BLOCK; }

bool hr_damping_ok(double zeta, double damp_mass, double damp_stiff) {
    // (written so that a NaN fails)
    return zeta >= 0.0 && damp_mass >= 0.0 && damp_stiff >= 0.0 && (zeta > 0.0 || damp_mass > 0.0 || damp_stiff > 0.0) &&
           zeta < INFINITY && damp_mass < INFINITY && damp_stiff < INFINITY;
}

int hr_sweep_launch(int B, int L, const TrsBatch& bt, const double* X, const double* lam, const int* n_mass, int p,
                    const double* g, const double* F, int S, const double* omega, double zeta, double damp_mass,
                    double damp_stiff, double* u_amp, int* u_at, double* R_amp, int* R_at, double* N_amp, int* N_at,
                    const int* mon_joint, int Pj, const int* mon_member, int Pm, double* frf_u, double* frf_N,
                    hipStream_t stream) {
    if (B <= 0) return 0;
    if (!hr_args_ok(L, p) || S < 1 || Pj < 0 || Pm < 0 || !hr_damping_ok(zeta, damp_mass, damp_stiff) ||
        !trs_hr_fits(bt.nJ_max, bt.nM_max, p) || bt.ld_f < 1 || X == nullptr || lam == nullptr || n_mass == nullptr ||
        g == nullptr || omega == nullptr || bt.free_index == nullptr || (bt.nJ_max > 0 && bt.xyz == nullptr) ||
        (frf_u != nullptr && Pj > 0 && mon_joint == nullptr) || (frf_N != nullptr && Pm > 0 && mon_member == nullptr))
        return (int)hipErrorInvalidValue;
    if (Pj == 0) frf_u = nullptr;
    if (Pm == 0) frf_N = nullptr;
    if (u_amp == nullptr && u_at == nullptr && R_amp == nullptr && R_at == nullptr && N_amp == nullptr &&
        N_at == nullptr && frf_u == nullptr && frf_N == nullptr)
        return 0;
    trs_lds::raise_lds_once<trs_hr_sweep_kernel>();
    hipLaunchKernelGGL(trs_hr_sweep_kernel, dim3(B, L), dim3(256), hr_lds(bt.nJ_max, bt.nM_max, p), stream, bt, L, X, lam,
                       n_mass, p, g, F, S, omega, zeta, damp_mass, damp_stiff, u_amp, u_at, R_amp, R_at, N_amp, N_at,
                       mon_joint, Pj, mon_member, Pm, frf_u, frf_N);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_hr_abi_version(void) { return TRS_HR_ABI_VERSION; }

int trs_hr_fits(int nJ_max, int nM_max, int p) {
    return nJ_max >= 0 && nM_max >= 0 && p >= 1 && p <= TRS_HR_MAX_MODES && hr_lds(nJ_max, nM_max, p) <= TRS_LDS_BYTES;
}

int trs_hr_modal(int B, int L, int nJ_max, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                 const double* X, int ld_f, const double* lam, const double* Mf, const int32_t* n_mass, int p,
                 const double* Pr, const double* ag, int residual, double* g, double* F, void* stream) {
    if (B <= 0) return 0;
    if (!hr_args_ok(L, p) || nJ_max < 0 || ld_f < 1 || free_index == nullptr || X == nullptr || lam == nullptr ||
        Mf == nullptr || n_mass == nullptr || (Pr == nullptr && ag == nullptr) || g == nullptr ||
        (residual && F == nullptr))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(trs_hr_modal_kernel, dim3(B, L), dim3(256), 0, (hipStream_t)stream,
                       trs_batch_dofs(nJ_max, free_index, n_free, nJ, nullptr, ld_f), L, X, lam, Mf, n_mass, p, Pr, ag,
                       residual, g, F);
    return (int)hipGetLastError();
}

int trs_hr_sweep(int B, int L, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E,
                 const double* A, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM,
                 const int32_t* joint_out, const double* X, int ld_f, const double* lam, const int32_t* n_mass, int p,
                 const double* g, const double* F, int S, const double* omega, double zeta, double damp_mass,
                 double damp_stiff, double* u_amp, int32_t* u_at, double* R_amp, int32_t* R_at, double* N_amp,
                 int32_t* N_at, const int32_t* mon_joint, int Pj, const int32_t* mon_member, int Pm, double* frf_u,
                 double* frf_N, void* stream) {
    if (B > 0 && nM_max > 0 && (conn == nullptr || E == nullptr || A == nullptr)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, n_free, nJ, nM,
                                  joint_out, ld_f);
    return hr_sweep_launch(B, L, bt, X, lam, n_mass, p, g, F, S, omega, zeta, damp_mass, damp_stiff, u_amp, u_at, R_amp,
                           R_at, N_amp, N_at, mon_joint, Pj, mon_member, Pm, frf_u, frf_N, (hipStream_t)stream);
}

int trs_hr_sweep_tab(int B, int L, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16,
                     const uint8_t* type_idx, const double* types, const int32_t* free_index, const int32_t* n_free,
                     const int32_t* nJ, const int32_t* nM, const int32_t* joint_out, const double* X, int ld_f,
                     const double* lam, const int32_t* n_mass, int p, const double* g, const double* F, int S,
                     const double* omega, double zeta, double damp_mass, double damp_stiff, double* u_amp, int32_t* u_at,
                     double* R_amp, int32_t* R_at, double* N_amp, int32_t* N_at, const int32_t* mon_joint, int Pj,
                     const int32_t* mon_member, int Pm, double* frf_u, double* frf_N, void* stream) {
    if (B > 0 && nM_max > 0 && (conn16 == nullptr || type_idx == nullptr || types == nullptr))
        return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free, nJ,
                                  nM, joint_out, ld_f);
    return hr_sweep_launch(B, L, bt, X, lam, n_mass, p, g, F, S, omega, zeta, damp_mass, damp_stiff, u_amp, u_at, R_amp,
                           R_at, N_amp, N_at, mon_joint, Pj, mon_member, Pm, frf_u, frf_N, (hipStream_t)stream);
}

}  // extern "C"
