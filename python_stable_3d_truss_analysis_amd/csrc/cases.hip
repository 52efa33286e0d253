// Several load cases of one factored batch (include/trs_solver.h "Load cases"): the factorisation that
// trs_potrf_batched left in the slab is reused for every right-hand side - the joint order, the assembly and
// the Cholesky factorisation are paid once per truss, not once per case.
//
//   trs_gather_cases   loads [B][L][nJ_max][3] (caller's joint numbering) -> reduced right-hand sides F [B][L][ld_f]
//   trs_potrs_cases    L y = f, then U x = y, for all L columns against the factored slab
//   trs_recover_cases  u, f_ext [B][L][nJ_max][3] and N [B][L][nM_max] of every case
//
// Substitution (measured: EXPERIMENTS.md R7.1): one wave per (truss, group of up to 16 cases).  Every 16 x 16 tile of the
// factor is read ONCE per direction per group and multiplied with the 16 x 16 block of the group's right-hand sides
// by four v_mfma_f64_16x16x4_f64 (16 rows x 16 cases).  The right-hand sides live in the f64 C/D layout throughout:
// lane l holds rows (l >> 4) + 4 r, case l & 15, in component r - which is also the B operand layout of the k-slice r,
// so a solved chunk feeds the next products from its registers.  Every element of the solution is read and written by
// ONE lane only (always the same lane and component), so the window needs no barriers.
// The window of the solution that is still being updated lives in LDS, as a ring of WC chunks (16 rows x 16 cases,
// 2 KB each): the forward pass is right-looking (after chunk q is solved, U[q, i]^T y_q is subtracted from the
// chunks q < i < cend[q]), the backward pass reads u_q, s < q < cend[s].  A matrix whose envelope reaches further
// than the ring holds works on its slice of F in global memory instead (same arithmetic, same bits).
#include "../../include/trs_solver.h"
#include "trs_common.h"
#include "trs_lds.h"

namespace {

using namespace trs_rec;

constexpr int CG = 16;  // cases per group = the N of the MFMA tile

#ifndef TRS_CASES_WINDOW
#define TRS_CASES_WINDOW 16  // chunks in the LDS ring (32 KB per wave)
#endif

// ---- gather ---------------------------------------------------------------------------------------------------------
// F[b][k][free_index[b][dof]] = loads[b][k][3 joint_in[b][j] + a] for the free DOFs (dof = 3 j + a), zero on the
// padding rows n_free[b] <= c < n_pad.  One work-group per (truss, case).
// (The batch's joint_out slot holds joint_in here: the same map, read the other way.)
__global__ __launch_bounds__(256) void trs_gather_cases_kernel(const TrsBatch bt, const int L,
                                                               const double* __restrict__ loads, double* __restrict__ F) {
    const int bk = blockIdx.x, b = bk / L, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const double* ld_case = loads + (size_t)bk * v.ndof_max;
    double* f = F + (size_t)bk * bt.ld_f;
    const int n = v.nfree, npad = min(trs_round_up(n, TRS_NB), bt.ld_f);
    for (int d = tid; d < v.ndof; d += 256) {
        const int r = v.row_of(d);
        if (r >= 0) f[r] = ld_case[3 * v.place(d / 3) + d % 3];
    }
    for (int c = n + tid; c < npad; c += 256) f[c] = 0.0;
}

// ---- substitution ---------------------------------------------------------------------------------------------------
typedef double cd4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ cd4 mfma16(double a, double b, cd4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__global__ __launch_bounds__(64) void trs_potrs_cases_kernel(const int L, const int ngroups,
                                                             const int* __restrict__ n_free, const int ld,
                                                             const size_t slab_stride, const double* __restrict__ S_all,
                                                             double* __restrict__ F_all, const int ld_f,
                                                             const int* __restrict__ env_all, const int n_pad_max,
                                                             const int wc) {
    extern __shared__ double ring[];  // [wc][16 rows][16 cases]
    const int b = blockIdx.x / ngroups, grp = blockIdx.x - b * ngroups;
    const int npad = trs_round_up(n_free[b], TRS_NB);
    if (npad == 0) return;
    const int nch = npad / 16;
    const int lane = threadIdx.x, li = lane & 15, lq = lane >> 4;
    const int k0 = grp * CG, ncase = min(CG, L - k0);
    const bool live = li < ncase;  // this lane's case exists
    const int* cend = env_all != nullptr ? trs_env_of(env_all, b, n_pad_max).cend : nullptr;
    // the stored extent of every row chunk, read once into LDS behind the ring (the loop bounds of every step), and the
    // widest window of either pass: chunks q .. (max_{q' <= q} cend[q']) - 1 are live at step q
    int* ce_s = reinterpret_cast<int*>(ring + (size_t)wc * 16 * CG);
    int w = 0;
    for (int t0 = 0, run = 0; t0 < nch; t0 += 64) {
        const int t = t0 + lane;
        const int v = t < nch ? (cend != nullptr ? min(cend[t], nch) : nch) : 0;
        if (t < nch) ce_s[t] = v;
        int m = v;  // running maximum (inclusive scan over the lanes)
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(m, off);
            if (lane >= off) m = max(m, up);
        }
        m = max(m, run);
        int wl = t < nch ? m - t : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) wl = max(wl, __shfl_xor(wl, off));
        w = max(w, wl);
        run = __shfl(m, 63);
    }
    __syncthreads();
    auto chunk_end = [&](int t) { return ce_s[t]; };
    const bool in_lds = w <= wc;
    const double* S = S_all + (size_t)b * slab_stride;
    double* Fc = F_all + ((size_t)b * L + k0 + (live ? li : 0)) * ld_f;  // this lane's case
    // element (row lq + 4 r, this lane's case) of chunk t of the window; the lanes of absent cases read zeros and
    // write nothing to F
    auto wget = [&](int t, int r) {
        return in_lds ? ring[((t % wc) * 16 + lq + 4 * r) * 16 + li] : (live ? Fc[16 * t + lq + 4 * r] : 0.0);
    };
    auto wput = [&](int t, int r, double v) {
        if (in_lds) ring[((t % wc) * 16 + lq + 4 * r) * 16 + li] = v;
        else if (live) Fc[16 * t + lq + 4 * r] = v;
    };
    auto load_f = [&](int t, cd4& v) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = live ? Fc[16 * t + lq + 4 * r] : 0.0;
    };
    // tile (row chunk c, column chunk i) in D form: component r = S[16 c + lq + 4 r][16 i + li]
    auto tile_d = [&](cd4& a, int c, int i) {
        const double* p = S + (size_t)(16 * c + lq) * ld + 16 * i + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = p[(size_t)4 * r * ld];
    };
    // the same tile in A form: component s = S[16 c + li][16 i + 4 s + lq]
    auto tile_a = [&](cd4& a, int c, int i) {
        const double* p = S + (size_t)(16 * c + li) * ld + 16 * i + lq;
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = p[4 * s];
    };

    // Everything a step reads from HBM that does not depend on the solution - the diagonal tile, the first PF
    // off-diagonal tiles of the row chunk and (forward) the chunks of F that enter the window - is requested one step
    // ahead, so that the chain of 2 nch steps does not wait for a memory latency at every step.
    constexpr int PF = 4;
    cd4 dg_n, a_n[PF], f_n[PF];
    int fin_lo = 0, fin_hi = 0;  // F chunks fin_lo .. fin_hi - 1 are in f_n

    // ---- forward: L y = f, right-looking.  inv(L_qq) is stored below the diagonal of the diagonal tile (its own
    // diagonal is 1 / U[c][c]); as the A operand, A[c][k] = inv(L)[c][k] (k <= c) sits at S[16 q + c][16 q + k].
    auto fetch_fwd = [&](int q, int hiw_now) {
        const int ce = chunk_end(q);
        tile_a(dg_n, q, q);
#pragma unroll
        for (int g = 0; g < PF; ++g)
            if (q + 1 + g < ce) tile_d(a_n[g], q, q + 1 + g);  // (component r = row lq + 4 r = k-slice r)
        fin_lo = hiw_now;
        fin_hi = in_lds ? min(ce, hiw_now + PF) : hiw_now;
#pragma unroll
        for (int g = 0; g < PF; ++g)
            if (fin_lo + g < fin_hi) load_f(fin_lo + g, f_n[g]);
    };
    int hiw = 0;  // chunks below hiw are in the window
    fetch_fwd(0, 0);
    for (int q = 0; q < nch; ++q) {
        const int ce = chunk_end(q);
        cd4 dg = dg_n, a0[PF];
#pragma unroll
        for (int g = 0; g < PF; ++g) a0[g] = a_n[g];
        if (in_lds) {
#pragma unroll
            for (int g = 0; g < PF; ++g)
                if (fin_lo + g < fin_hi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) wput(fin_lo + g, r, f_n[g][r]);
            hiw = max(hiw, fin_hi);
            for (; hiw < ce; ++hiw) {  // (more chunks than were requested ahead)
                cd4 v;
                load_f(hiw, v);
#pragma unroll
                for (int r = 0; r < 4; ++r) wput(hiw, r, v[r]);
            }
        }
        if (q + 1 < nch) fetch_fwd(q + 1, hiw);
        cd4 fq;
#pragma unroll
        for (int r = 0; r < 4; ++r) fq[r] = wget(q, r);
        cd4 y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 4 * s + lq;  // A[li][k]
            const double a = k < li ? dg[s] : (k == li ? 1.0 / dg[s] : 0.0);
            y = mfma16(a, fq[s], y);
        }
        // y_q is final: to F (the backward pass starts from it)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (live) Fc[16 * q + lq + 4 * r] = y[r];
        // f_i -= U[q, i]^T y_q for the chunks of row chunk q's envelope; A[c][k] = U[16 q + k][16 i + c]
        for (int i0 = q + 1; i0 < ce; i0 += PF) {
            cd4 a[PF];
            if (i0 == q + 1) {
#pragma unroll
                for (int g = 0; g < PF; ++g) a[g] = a0[g];
            } else {
#pragma unroll
                for (int g = 0; g < PF; ++g)
                    if (i0 + g < ce) tile_d(a[g], q, i0 + g);
            }
#pragma unroll
            for (int g = 0; g < PF; ++g) {
                if (i0 + g >= ce) break;
                cd4 d = {0.0, 0.0, 0.0, 0.0};
                // tile_d gives S[16q + lq + 4r][16i + li] = A[li][lq + 4r]: the A operand wants A[li][4 s + lq] - the
                // same element with r = s
#pragma unroll
                for (int s = 0; s < 4; ++s) d = mfma16(a[g][s], y[s], d);
#pragma unroll
                for (int r = 0; r < 4; ++r) wput(i0 + g, r, wget(i0 + g, r) - d[r]);
            }
        }
    }
    // ---- backward: U x = y.  t_s = y_s - sum_{s < q < cend[s]} U[s, q] x_q, then x_s = inv(L_ss)^T t_s.
    // The diagonal tile in D form: component r = S[16 s + lq + 4 r][16 s + li] = inv(L)[k = lq + 4 r][c = li] (k > c);
    // the off-diagonal tiles in A form: A[c][k] = U[16 s + c][16 q + k]; y_s from F (this lane's elements).
    auto fetch_bwd = [&](int s) {
        const int ce = chunk_end(s);
        tile_d(dg_n, s, s);
#pragma unroll
        for (int g = 0; g < PF; ++g)
            if (s + 1 + g < ce) tile_a(a_n[g], s, s + 1 + g);
        load_f(s, f_n[0]);
    };
    fetch_bwd(nch - 1);
    for (int s = nch - 1; s >= 0; --s) {
        const int ce = chunk_end(s);
        cd4 dg = dg_n, t = f_n[0], a0[PF];
#pragma unroll
        for (int g = 0; g < PF; ++g) a0[g] = a_n[g];
        if (s > 0) fetch_bwd(s - 1);
        cd4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int q0 = s + 1; q0 < ce; q0 += PF) {
            cd4 a[PF];
            if (q0 == s + 1) {
#pragma unroll
                for (int g = 0; g < PF; ++g) a[g] = a0[g];
            } else {
#pragma unroll
                for (int g = 0; g < PF; ++g)
                    if (q0 + g < ce) tile_a(a[g], s, q0 + g);
            }
#pragma unroll
            for (int g = 0; g < PF; ++g) {
                if (q0 + g >= ce) break;
                cd4 xq;
#pragma unroll
                for (int r = 0; r < 4; ++r) xq[r] = wget(q0 + g, r);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = mfma16(a[g][k], xq[k], acc);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) t[r] -= acc[r];
        cd4 x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = lq + 4 * r;  // A[li][k] = inv(L)^T[li][k] = inv(L)[k][li]
            const double a = k > li ? dg[r] : (k == li ? 1.0 / dg[r] : 0.0);
            x = mfma16(a, t[r], x);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (in_lds) wput(s, r, x[r]);
            if (live) Fc[16 * s + lq + 4 * r] = x[r];
        }
    }
}

// ---- recovery -------------------------------------------------------------------------------------------------------
struct RecoverTables : EndLists {   // (the member-end lists of the constrained joints: trs_recover.h)
    double* u;   // [3 nJ_max]  displacements of one case, device numbering
};

template <class Arena>
__host__ __device__ inline RecoverTables recover_layout(Arena& a, int nJ_max, int nM_max) {
    RecoverTables t;
    t.u = a.template take<double>(3, nJ_max);
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    return t;
}

// trs_recover's staged path (recover.hip) with the truss's tables built once and a loop over the cases: the member-end
// lists of the constrained joints are counting-sorted once, then per case u is staged in LDS (device numbering),
// N and the reactions are formed by the SAME functions (trs_recover.h) in the same order, and u / f_ext go out through
// joint_out.  f_ext at a free DOF is the case's applied load.  One work-group per truss.
__global__ __launch_bounds__(256) void trs_recover_cases_kernel(const TrsBatch bt, const int L,
                                                                const double* __restrict__ loads,
                                                                const double* __restrict__ F, double* __restrict__ u_out,
                                                                double* __restrict__ f_out, double* __restrict__ N_out) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max, ld_f = bt.ld_f, ndof_max = v.ndof_max;
    trs_lds::Carve lds(sh);
    const RecoverTables t = recover_layout(lds, nJ_max, nM_max);
    double* u = t.u;
    // sorted by member id once (joint_reaction sorts in place; later cases find the lists sorted); the case loop opens
    // with the barrier that the builder leaves to its caller
    build_end_lists(t, v, tid, [&](int j) { return v.any_held(j); });
    for (int k = 0; k < L; ++k) {
        const size_t bk = (size_t)b * L + k;
        const double* fk = F + bk * ld_f;
        const double* lk = loads + bk * ndof_max;      // caller's numbering
        double* uo = u_out + bk * ndof_max;
        double* fo = f_out + bk * ndof_max;
        __syncthreads();  // (the previous case's readers of u are done)
        for (int d = tid; d < ndof_max; d += 256) {
            const int r = v.row_of(d);
            const double val = r >= 0 ? fk[r] : 0.0;
            u[d] = val;
            const int o = 3 * v.place(d / 3) + d % 3;
            uo[o] = val;
            if (r >= 0) fo[o] = lk[o];                    // free DOF: the applied load
            else if (d >= v.ndof) fo[o] = 0.0;            // padding
        }
        __syncthreads();
        for (int m = tid; m < nM_max; m += 256) {
            double axial = 0.0;
            if (m < v.members) {
                const int2 c = v.ends(m).c;
                const MemberGeom g = member_geom(v.X, c.x, c.y);
                axial = member_axial(g, v.mem.EA(v.mbase + m), u, c.x, c.y);
            }
            N_out[bk * nM_max + m] = axial;
        }
        for (int j = tid; j < v.joints; j += 256) {
            const int deg = t.cnt[j];
            double r[3] = {0.0, 0.0, 0.0};   // (a constrained joint without members: zero reaction)
            if (deg == 0 && !v.any_held(j)) continue;
            if (deg != 0) joint_reaction(t.ends + t.start[j], deg, v, u, r);
            const int o = 3 * v.place(j);
            const TrussView::Rows rows = v.rows(j);   // (read here, behind the reaction: fewer scalars live across it)
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (rows.held(a)) fo[o + a] = r[a];
        }
    }
}

}  // namespace

int trs_gather_cases_launch(int B, const TrsBatch& bt, int L, const double* loads, double* F, hipStream_t stream) {
    if (B <= 0 || L <= 0) return 0;
    hipLaunchKernelGGL(trs_gather_cases_kernel, dim3((unsigned)B * (unsigned)L), dim3(256), 0, stream, bt, L, loads, F);
    return (int)hipGetLastError();
}

extern "C" int trs_potrs_cases_launch(int B, int L, const int* n_free, int ld, size_t slab_stride, int n_pad_max,
                                      const double* S, double* F, int ld_f, const int* env, hipStream_t stream) {
    if (B <= 0 || L <= 0 || n_pad_max <= 0) return 0;
    if (ld_f < n_pad_max) return (int)hipErrorInvalidValue;
    const int ngroups = (L + CG - 1) / CG;
    const int wc = min(n_pad_max / 16, TRS_CASES_WINDOW);
    const size_t lds = (size_t)wc * 16 * CG * sizeof(double) + (size_t)(n_pad_max / 16) * sizeof(int);
    if (lds > 64 * 1024) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(trs_potrs_cases_kernel, dim3((unsigned)B * (unsigned)ngroups), dim3(64), lds, stream, L, ngroups,
                       n_free, ld, slab_stride, S, F, ld_f, env, n_pad_max, wc);
    return (int)hipGetLastError();
}

extern "C" size_t trs_recover_cases_lds(int nJ_max, int nM_max) {
    return trs_lds::count([&](auto& a) { recover_layout(a, nJ_max, nM_max); });
}

int trs_recover_cases_launch(int B, const TrsBatch& bt, int L, const double* loads, const double* F, double* u,
                             double* f_ext, double* N, hipStream_t stream) {
    if (B <= 0 || L <= 0) return 0;
    const size_t lds = trs_recover_cases_lds(bt.nJ_max, bt.nM_max);
    if (lds > TRS_LDS_BYTES) return (int)hipErrorInvalidValue;
    trs_lds::raise_lds_once<trs_recover_cases_kernel>();
    hipLaunchKernelGGL(trs_recover_cases_kernel, dim3(B), dim3(256), lds, stream, bt, L, loads, F, u, f_ext, N);
    return (int)hipGetLastError();
}
