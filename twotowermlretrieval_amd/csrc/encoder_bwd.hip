// K7: gradient of RNNEncoder.forward w.r.t. every trainable tensor (what loss.backward() computes
// through backend/model.py:48-75; backend/main.py:254).  The embedding table is frozen
// (model.py:25-27) and receives no gradient.
//
//   head_bwd   F.normalize backward, then (bidirectional) the Linear(2H,H) backward as GEMMs
//   gru_bwd    reverse-time recurrence: one workgroup = the same 16 batch rows as the forward; the
//              gate derivatives are lane-local (they reuse the r,z,n,W_hn h stash the forward wrote),
//              dh_{t-1} = dh_t z + dGh W_hh runs on v_mfma_f32_16x16x4_f32 with dGh staged in LDS and
//              W_hh streamed from L2 in a pre-packed (transposed) B-operand order
//   weights    dW_ih = dGi^T X, dW_hh = dGh^T H_prev over ALL tokens at once: split-K fp32 MFMA GEMMs
//              with a deterministic slab reduction; X rows are gathered from the embedding table and
//              H_prev rows are addressed through a "previous token" index map (no copies)
#include "encoder.h"
#include "sgemm.h"

#include <stdlib.h>

namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float fast_tanh_b(float x) { return tt_fast_tanh(x); } // the forward's tanh: tanh(c_t) is the value h_t used

// d_hid = backward of y = hid / max(|hid|, 1e-12) (or identity)
// (block 0 also clears `zero_words`: the 16 scale words of this call's f16-split weight-gradient products, which the kernels
//  behind this one raise with atomicMax -- a separate launch before)
__global__ __launch_bounds__(256) void head_bwd_kernel(const float *__restrict__ hid, const float *__restrict__ d_out,
                                                       int H, int normalize, float *__restrict__ d_hid, unsigned *zero_words)
{
    __shared__ float red[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b == 0 && tid < 16)
        zero_words[tid] = 0u;
    const float *x = hid + (size_t)b * H, *dy = d_out + (size_t)b * H;
    if (!normalize) {
        for (int u = tid; u < H; u += 256)
            d_hid[(size_t)b * H + u] = dy[u];
        return;
    }
    float ss = 0.0f, dt = 0.0f;
    for (int u = tid; u < H; u += 256) {
        ss += x[u] * x[u];
        dt += x[u] * dy[u];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        ss += __shfl_xor(ss, off);
        dt += __shfl_xor(dt, off);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = ss;
        red[4 + (tid >> 6)] = dt;
    }
    __syncthreads();
    const float nrm = sqrtf(red[0] + red[1] + red[2] + red[3]);
    const float dot = red[4] + red[5] + red[6] + red[7]; // x . dy
    for (int u = tid; u < H; u += 256) {
        float g;
        if (nrm < 1e-12f)
            g = dy[u] / 1e-12f;
        else
            g = (dy[u] - (x[u] / nrm) * (dot / nrm)) / nrm;
        d_hid[(size_t)b * H + u] = g;
    }
}

// column sums of X[m][n], m < *m_dyn, split over gridDim.y row slices -> slabs[y][n]; optionally the bit pattern of
// max |X| over the same elements -> *absmax (atomicMax; zeroed by the caller): the scale of the f16-split GEMMs
// that consume X next, for the price of this pass
__global__ __launch_bounds__(256) void colsum_kernel(const float *__restrict__ X, int64_t ld, int N, int M,
                                                     const int *__restrict__ m_dyn, float *__restrict__ slabs,
                                                     unsigned *__restrict__ absmax)
{
    const int Me = m_dyn ? min(M, *m_dyn) : M;
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int per = (Me + gridDim.y - 1) / gridDim.y;
    const int m0 = blockIdx.y * per, m1 = min(m0 + per, Me);
    float s = 0.0f, mx = 0.0f;
    if (n < N) {
        int m = m0;
        for (; m + 4 <= m1; m += 4) { // four loads in flight; the sum keeps its row order
            const float a = X[(size_t)m * ld + n], b = X[(size_t)(m + 1) * ld + n];
            const float c = X[(size_t)(m + 2) * ld + n], d = X[(size_t)(m + 3) * ld + n];
            s += a;
            s += b;
            s += c;
            s += d;
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(a), fabsf(b))), fmaxf(fabsf(c), fabsf(d)));
        }
        for (; m < m1; ++m) {
            const float a = X[(size_t)m * ld + n];
            s += a;
            mx = fmaxf(mx, fabsf(a));
        }
        slabs[(size_t)blockIdx.y * N + n] = s;
    }
    if (absmax) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            mx = fmaxf(mx, __shfl_xor(mx, off));
        if ((threadIdx.x & 63) == 0 && mx > 0.0f)
            atomicMax(absmax, __float_as_uint(mx));
    }
}

// wtp[((w*2 + ct)*(GH/16) + c)*256 + lane*4 + e] = W_hh[16c + 4(lane>>4) + e][32w + 16ct + (lane&15)],  GH = ng*H rows
__global__ __launch_bounds__(256) void pack_whh_t_kernel(const float *__restrict__ W, int H, int ng, float *__restrict__ wtp)
{
    const int n = ng * H * H / 4;
    const int nc = ng * H / 16;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int lane = i & 63;
        int r = i >> 6;
        const int c = r % nc;
        r /= nc;
        const int ct = r & 1, w = r >> 1;
        const int col = 32 * w + 16 * ct + (lane & 15);
        const int row = 16 * c + 4 * (lane >> 4);
        f32x4v v;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            v[e] = W[(size_t)(row + e) * H + col];
        *(f32x4v *)(wtp + (size_t)i * 4) = v;
    }
}

// (GruBwdDir / GruBwdParams: encoder.h)

// CELL_GRU: dGh = [dr_pre, dz_pre, dn_pre r], dh_{t-1} = dh z + dGh W_hh.   CELL_LSTM: dG = [di_pre, df_pre, dg_pre,
// do_pre] (the same for the input and the hidden side), dh_{t-1} = dG W_hh, dc carried in registers.   CELL_RNN:
// dG = dh (1 - h'^2), dh_{t-1} = dG W_hh.
template <int MAXW, int CELL>
__global__ __launch_bounds__(MAXW * 64) void gru_bwd_seq_kernel(GruBwdParams p)
{
    const uint64_t drop_seed_v = (p.drop_p > 0.0f && p.drop_seed_ptr) ? *p.drop_seed_ptr : p.drop_seed;
    constexpr int NG = CELL == CELL_LSTM ? 4 : (CELL == CELL_RNN ? 1 : 3);
    extern __shared__ __attribute__((aligned(16))) float gt[]; // [16][NG*H+4]
    const GruBwdDir d = p.dir[blockIdx.y];
    const int H = p.H, HG = NG * H, LDG = NG * H + 4, nc = HG / 16;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * ENC_RB;

    int len_e[4], off_e[4], rid_e[4], unit[2];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int br = row0 + kq * 4 + e;
        rid_e[e] = br < p.B ? p.perm[br] : -1;
        len_e[e] = rid_e[e] >= 0 ? p.len[rid_e[e]] : 0;
        off_e[e] = rid_e[e] >= 0 ? p.tok_off[rid_e[e]] : 0;
    }
    int steps = max(max(len_e[0], len_e[1]), max(len_e[2], len_e[3]));
    steps = max(steps, __shfl_xor(steps, 16));
    steps = max(steps, __shfl_xor(steps, 32));
    float dh[2][4];
    float dc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}; // LSTM: gradient w.r.t. the cell state
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        unit[ct] = 32 * w + 16 * ct + j;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            dh[ct][e] = (d.d_hfin && rid_e[e] >= 0) ? d.d_hfin[(size_t)rid_e[e] * H + unit[ct]] : 0.0f;
    }
    const float *wbase = d.wtp + (size_t)w * 2 * nc * 256 + lane * 4;

    // The stash of a step is loaded one step AHEAD, so the global latency hides under the previous step's MFMA loop
    // instead of sitting on the serial path of every step.  GRU: r,z,n,ghn,h_{t-1}.  LSTM: i,f,g,o in r,z,n,ghn,
    // c_{t-1} in hp, c_t in cn.  RNN: h_t in r.
    struct Stash {
        float r[2][4], z[2][4], n[2][4], ghn[2][4], hp[2][4], cn[2][4], dsv[2][4];
    };
    auto load_stash = [&](int s, Stash &st) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool a = s >= 0 && s < len_e[e];
            const int t = d.reverse ? len_e[e] - 1 - s : s;
            const size_t tok = (size_t)(off_e[e] + (a ? t : 0));
            const size_t ptok = d.reverse ? tok + 1 : tok - 1;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int u = unit[ct];
                st.r[ct][e] = st.z[ct][e] = st.n[ct][e] = st.ghn[ct][e] = st.hp[ct][e] = st.cn[ct][e] = st.dsv[ct][e] = 0.0f;
                if (a) {
                    if constexpr (CELL != CELL_RNN) {
                        const float *gs = d.gates + tok * 4 * H + u;
                        st.r[ct][e] = gs[0];
                        st.z[ct][e] = gs[H];
                        st.n[ct][e] = gs[2 * H];
                        st.ghn[ct][e] = gs[3 * H];
                    } else {
                        st.r[ct][e] = d.hseq[tok * p.ld + d.col0 + u];
                    }
                    if constexpr (CELL == CELL_GRU) {
                        if (s > 0)
                            st.hp[ct][e] = d.hseq[ptok * p.ld + d.col0 + u];
                    }
                    if constexpr (CELL == CELL_LSTM) {
                        st.cn[ct][e] = d.cseq[tok * H + u];
                        if (s > 0)
                            st.hp[ct][e] = d.cseq[ptok * H + u];
                    }
                    if (d.d_seq)
                        st.dsv[ct][e] = d.d_seq[tok * p.ld + d.col0 + u];
                }
            }
        }
    };
    Stash cur_st, next_st;
    load_stash(steps - 1, cur_st);

    for (int s = steps - 1; s >= 0; --s) {
        bool act[4];
        float direct[2][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            act[e] = s < len_e[e];
            const int t = d.reverse ? len_e[e] - 1 - s : s;
            const size_t tok = (size_t)(off_e[e] + (act[e] ? t : 0));
            float *grow = gt + (kq * 4 + e) * LDG;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int u = unit[ct];
                float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f; // this lane's elements of dGh
                direct[ct][e] = 0.0f;
                if (act[e]) {
                    float dsv = cur_st.dsv[ct][e];
                    if (d.d_seq && p.drop_p > 0.0f)
                        dsv *= tt_dropout_scale(drop_seed_v, p.drop_layer,
                                                ((uint64_t)rid_e[e] * p.T + t) * p.ld + d.col0 + u, p.drop_p);
                    const float dhv = dh[ct][e] + dsv;
                    float *go = d.dgi + tok * HG + u;
                    if constexpr (CELL == CELL_GRU) {
                        const float r = cur_st.r[ct][e], z = cur_st.z[ct][e], n = cur_st.n[ct][e], ghn = cur_st.ghn[ct][e];
                        const float hp = cur_st.hp[ct][e];
                        const float dn_pre = dhv * (1.0f - z) * (1.0f - n * n);
                        g1 = dhv * (hp - n) * z * (1.0f - z);
                        g0 = dn_pre * ghn * r * (1.0f - r);
                        g2 = dn_pre * r;
                        direct[ct][e] = dhv * z;
                        go[0] = g0;
                        go[H] = g1;
                        go[2 * H] = dn_pre;
                        float *gh = d.dghn + tok * HG + u; // dGh differs from dGi in the n column only; kept whole so
                        gh[0] = g0;                        // that dW_hh and db_hh are ONE product / column sum each
                        gh[H] = g1;
                        gh[2 * H] = g2;
                    } else if constexpr (CELL == CELL_LSTM) {
                        const float ig = cur_st.r[ct][e], fg = cur_st.z[ct][e], gg = cur_st.n[ct][e], og = cur_st.ghn[ct][e];
                        const float cp = cur_st.hp[ct][e];
                        const float tc = fast_tanh_b(cur_st.cn[ct][e]);
                        const float dct = dc[ct][e] + dhv * og * (1.0f - tc * tc);
                        g0 = dct * gg * ig * (1.0f - ig);
                        g1 = dct * cp * fg * (1.0f - fg);
                        g2 = dct * ig * (1.0f - gg * gg);
                        g3 = dhv * tc * og * (1.0f - og);
                        dc[ct][e] = dct * fg;
                        go[0] = g0;
                        go[H] = g1;
                        go[2 * H] = g2;
                        go[3 * H] = g3;
                    } else {
                        const float hn = cur_st.r[ct][e];
                        g0 = dhv * (1.0f - hn * hn);
                        go[0] = g0;
                    }
                }
                grow[u] = g0;
                if constexpr (NG > 1)
                    grow[H + u] = g1;
                if constexpr (NG > 2)
                    grow[2 * H + u] = g2;
                if constexpr (NG > 3)
                    grow[3 * H + u] = g3;
            }
        }
        load_stash(s - 1, next_st); // in flight during the MFMA loop below
        __syncthreads();
        f32x4v acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        const float *gA = gt + j * LDG + 4 * kq;
        for (int c = 0; c < nc; ++c) {
            const f32x4v a = *(const f32x4v *)(gA + 16 * c);
            const f32x4v b0 = *(const f32x4v *)(wbase + (size_t)c * 256);
            const f32x4v b1 = *(const f32x4v *)(wbase + ((size_t)nc + c) * 256);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b0[e], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b1[e], acc[1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (act[e])
                    dh[ct][e] = direct[ct][e] + acc[ct][e];
        cur_st = next_st;
        __syncthreads();
    }
}

template <int CELL>
int launch_bwd_seq(const GruBwdParams &bp, int B, int H, int ndir, size_t lds, hipStream_t st)
{
    if (lds > 48 * 1024) {
        TT_HIP_CHECK(hipFuncSetAttribute((const void *)gru_bwd_seq_kernel<8, CELL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        TT_HIP_CHECK(hipFuncSetAttribute((const void *)gru_bwd_seq_kernel<16, CELL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    if (H <= 256)
        hipLaunchKernelGGL((gru_bwd_seq_kernel<8, CELL>), dim3((B + ENC_RB - 1) / ENC_RB, ndir), dim3(H / 32 * 64), lds, st, bp);
    else
        hipLaunchKernelGGL((gru_bwd_seq_kernel<16, CELL>), dim3((B + ENC_RB - 1) / ENC_RB, ndir), dim3(H / 32 * 64), lds, st, bp);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

// g_table[ids[m]][c] += dx[m][c] for the valid tokens m with ids[m] != 0 (float atomics at the memory side)
__global__ __launch_bounds__(256) void table_scatter_kernel(const float *__restrict__ dx, const int32_t *__restrict__ ids,
                                                            const int *__restrict__ m_dyn, int M, int E,
                                                            float *__restrict__ g_table)
{
    const int Me = min(M, *m_dyn);
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63, nw = gridDim.x * 4;
    for (int m = wave; m < Me; m += nw) {
        const int id = ids[m];
        if (id == 0)
            continue;
        for (int c = lane; c < E; c += 64)
            atomicAdd(g_table + (size_t)id * E + c, dx[(size_t)m * E + c]);
    }
}

// out_ih[c] = sum over row groups of slab[g][c], out_hh[c] = ... of slab[g][n + c].  A block takes 32 columns x 8 parts:
// part p adds its eighth of the row groups in order, the 8 partial sums are combined in part order (fixed order, so the
// result does not depend on the launch; one thread walking all groups of a column was 64 dependent loads, 12-19 us).
__global__ __launch_bounds__(256) void bias_reduce_kernel(const float *__restrict__ slab, int ngroups, int n,
                                                          float *__restrict__ out_ih, float *__restrict__ out_hh)
{
    __shared__ float part[8][32];
    const int col = threadIdx.x & 31, p = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + col;
    const int per = (ngroups + 7) / 8;
    float s = 0.0f;
    if (c < 2 * n)
        for (int g = p * per; g < min((p + 1) * per, ngroups); ++g)
            s += slab[(size_t)g * 2 * n + c];
    part[p][col] = s;
    __syncthreads();
    if (p == 0 && c < 2 * n) {
        float t = part[0][col];
#pragma unroll
        for (int q = 1; q < 8; ++q)
            t += part[q][col];
        if (c < n)
            out_ih[c] = t;
        else
            out_hh[c - n] = t;
    }
}

constexpr int COLSUM_SLICES = 256; // N <= 3H <= 1536 columns: 256 x N floats fit the split-K slab buffer

// out[n] = column sums of X[M][N] (row pitch N; rows clipped by *m_dyn when given); absmax (nullable): see colsum_kernel
struct ColSum {
    const float *X;
    int N, M;
    const int *m_dyn;
    float *out;
    unsigned *absmax;
};
int colsum(const ColSum &s, float *slabs, hipStream_t st)
{
    hipLaunchKernelGGL(colsum_kernel, dim3((s.N + 255) / 256, COLSUM_SLICES), dim3(256), 0, st, s.X, (int64_t)s.N, s.N, s.M, s.m_dyn,
                       slabs, s.absmax);
    TT_LAUNCH_CHECK();
    return tt_slab_reduce(slabs, COLSUM_SLICES, s.N, s.out, 0, st);
}

// what the reductions over all tokens of a call share: the split-K scratch, the bound MT of the token count and the device
// word that holds the count itself
struct SplitK {
    float *slabs;
    int MT;
    const int *m_valid;
    hipStream_t st;
};

// out[Mo][No] = A^T * B, both summed over the tokens, split-K + deterministic reduce.
// a_absmax != nullptr: on the f16 pipes (fp16 hi/lo split of both operands, sgemm.h): A = gradients, scaled by the
// power of two that *a_absmax (max |A|, from the recurrence kernel or the colsum pass over the same matrix) implies; B scaled
// by the power of two of *b_absmax when given, else by 2^b_exp.
// b_rows: an upper bound of B's row count (the 256-row-tile kernel addresses B with 32-bit offsets and checks it).
struct GemmTn {
    const float *A; // [tokens][lda]
    int64_t lda;
    int Mo;
    const float *B; // [b_rows][ldb], the row of token k: b_map ? b_map[k] : k
    int64_t ldb;
    const int32_t *b_map;
    int64_t b_rows;
    int No;
    const unsigned *a_absmax;
    int b_exp;
    const unsigned *b_absmax;
    float *out;
};
int gemm_tn(const GemmTn &t, const SplitK &k)
{
    SgemmParams g;
    g.A = t.A;
    g.B = t.B;
    g.C = k.slabs;
    g.b_map = t.b_map;
    g.k_dyn = k.m_valid;
    g.M = t.Mo;
    g.N = t.No;
    g.K = k.MT;
    g.lda = t.lda;
    g.ldb = t.ldb;
    g.ldc = t.No;
    g.slab_stride = (int64_t)t.Mo * t.No;
    g.a_absmax = t.a_absmax;
    g.b_absmax = t.a_absmax ? t.b_absmax : nullptr;
    g.b_exp = t.b_exp;
    if (t.a_absmax && tt_wgrad16_supported(t.Mo, t.No, t.lda, t.ldb, t.b_rows) && !((uintptr_t)t.A & 15) && !((uintptr_t)t.B & 15)) {
        // 256-row output tiles with the whole K slab in one workgroup per CU (wgrad16.hip)
        const int ns = tt_wgrad16_slabs(t.Mo, t.No, tt_device_cus(), ENC_SPLITK);
        TT_RC_CHECK(tt_wgrad16(g, ns, k.st));
        return tt_slab_reduce(k.slabs, ns, (int64_t)t.Mo * t.No, t.out, 0, k.st);
    }
    TT_RC_CHECK(t.a_absmax ? tt_sgemm16(g, true, true, ENC_SPLITK, k.st) : tt_sgemm(g, true, true, ENC_SPLITK, k.st));
    return tt_slab_reduce(k.slabs, ENC_SPLITK, (int64_t)t.Mo * t.No, t.out, 0, k.st);
}

} // namespace

// ------------------------------------------------------------------ the steps of one backward call
// (lengths, token offsets, row order, packed ids and the "previous token" maps are the training forward's: csrc/encoder.hip)
static SplitK bwd_splitk(const EncCall &c, const EncLayout &lo)
{
    char *ws = (char *)c.workspace;
    return {(float *)(ws + lo.slabs), (int)lo.MT, (const int32_t *)(ws + lo.tok_off) + c.B, c.st};
}
static unsigned *bwd_flag(const EncCall &c, const EncLayout &lo) { return (unsigned *)((char *)c.workspace + lo.flag); }
// the scale words of layer l, direction d's weight-gradient products (max |dGi|; max |dGh| behind it): null on the fp32-MFMA path
static unsigned *bwd_dg_max(const EncCall &c, const EncLayout &lo, int l, int d)
{
    return c.o.force_f32 ? nullptr : bwd_flag(c, lo) + enc_flag_dgi_max(l, d);
}

// head: F.normalize backward (the kernel also clears the ENC_FLAG_DG_WORDS maxima that the kernels behind it raise), then
// (bidirectional) the Linear(2H, H) backward
static int bwd_head(const EncCall &c, const EncLayout &lo)
{
    char *ws = (char *)c.workspace;
    const int B = c.B, H = c.H;
    hipStream_t st = c.st;
    float *slabs = (float *)(ws + lo.slabs);
    float *d_hfin = (float *)(ws + lo.d_hfin), *d_hid = (float *)(ws + lo.d_hid);
    const float *hfin = (const float *)(ws + lo.hfin);
    hipLaunchKernelGGL(head_bwd_kernel, dim3(B), dim3(256), 0, st, (const float *)(ws + lo.hid), c.bwd->d_out, H, c.normalize,
                       c.bidirectional ? d_hid : d_hfin, bwd_flag(c, lo) + ENC_FLAG_DG);
    TT_LAUNCH_CHECK();
    if (!c.bidirectional)
        return TT_OK;
    TT_RC_CHECK(colsum({d_hid, H, B, nullptr, c.bwd->g_proj_b, nullptr}, slabs, st));
    for (int d = 0; d < 2; ++d) {
        // g_proj_w[:, dH:(d+1)H] = d_hid^T * hfin[d]
        SgemmParams g;
        g.A = d_hid;
        g.B = hfin + (size_t)d * B * H;
        g.M = g.N = H;
        g.K = B;
        g.lda = g.ldb = H;
        // The product sums over the B batch rows: with one k-range a 256 x 256 output is 4 workgroups walking B / 32
        // tiles each (160 us at B = 1024).  Split it over 16 k-ranges into contiguous slabs, reduce in fixed order,
        // then place the H x H block into its half of g_proj_w (row pitch 2H).
        const int psplit = B >= 256 ? 16 : 1;
        if (psplit > 1) {
            float *ptmp = slabs + (size_t)psplit * H * H; // behind the slabs, inside the split-K scratch
            g.C = slabs;
            g.ldc = H;
            g.slab_stride = (int64_t)H * H;
            TT_RC_CHECK(tt_sgemm(g, true, true, psplit, st));
            TT_RC_CHECK(tt_slab_reduce(slabs, psplit, (int64_t)H * H, ptmp, 0, st));
            TT_HIP_CHECK(hipMemcpy2DAsync(c.bwd->g_proj_w + (size_t)d * H, sizeof(float) * 2 * H, ptmp, sizeof(float) * H,
                                          sizeof(float) * H, H, hipMemcpyDeviceToDevice, st));
        } else {
            g.C = c.bwd->g_proj_w + (size_t)d * H;
            g.ldc = 2 * H;
            TT_RC_CHECK(tt_sgemm(g, true, true, 1, st));
        }
        // d_hfin[d] = d_hid * proj_w[:, dH:(d+1)H]
        SgemmParams h;
        h.A = d_hid;
        h.B = c.proj_w + (size_t)d * H;
        h.C = d_hfin + (size_t)d * B * H;
        h.M = B;
        h.N = h.K = H;
        h.lda = h.ldc = H;
        h.ldb = 2 * H;
        TT_RC_CHECK(tt_sgemm(h, false, true, 1, st));
    }
    return TT_OK;
}

// the reverse-time recurrence of layer l, both directions, behind the transposed pack of W_hh; tt_enc_sync_t as in the
// forward: wait in front of the call's first recurrence launch (the top layer's), record behind its last (layer 0's)
static int bwd_recurrence(const EncCall &c, const EncLayout &lo, const EncRoute &r, int l)
{
    char *ws = (char *)c.workspace;
    const int B = c.B, H = c.H, ndir = lo.ndir, NG = lo.ng, H3 = NG * H; // H3: gate rows (3H for the GRU)
    hipStream_t st = c.st;
    const bool top = l == c.L - 1;
    const int n_rowgroups = (B + ENC_RB - 1) / ENC_RB;
    float *slabs = (float *)(ws + lo.slabs);
    GruBwdParams bp;
    bp.len = (const int32_t *)(ws + lo.len);
    bp.tok_off = (const int32_t *)(ws + lo.tok_off);
    bp.perm = (const int32_t *)(ws + lo.perm);
    bp.B = B;
    bp.H = H;
    bp.ld = ndir * H;
    bp.drop_p = (r.drop && !top) ? c.dropout_p : 0.0f;
    bp.drop_seed = c.o.seed;
    bp.drop_seed_ptr = c.o.seed_dev;
    bp.drop_layer = l;
    bp.T = c.T;
    for (int d = 0; d < ndir; ++d) {
        const float *const *w = c.weights + ((size_t)l * ndir + d) * 4;
        // max |W_hh| of this layer and direction: the training forward left it in its status block (encoder.hip)
        const unsigned *wmax = bwd_flag(c, lo) + enc_flag_whh_max(l, d);
        if (r.use16) {
            TT_RC_CHECK(gru16_pack_t(w[1], H, wmax, ws + lo.wtp[d], st));
        } else {
            hipLaunchKernelGGL(pack_whh_t_kernel, dim3(96), dim3(256), 0, st, w[1], H, NG, (float *)(ws + lo.wtp[d]));
        }
        GruBwdDir &bd = bp.dir[d];
        bd.wmax = wmax;
        bd.gates = (const float *)(ws + lo.gates[l][d]);
        bd.cseq = c.cell == CELL_LSTM ? (const float *)(ws + lo.cseq[l][d]) : nullptr;
        bd.hseq = (const float *)(ws + lo.x[l + 1]);
        bd.d_seq = top ? nullptr : (const float *)(ws + lo.dx[(l + 1) & 1]);
        bd.d_hfin = top ? (float *)(ws + lo.d_hfin) + (size_t)d * B * H : nullptr;
        bd.wtp = (const float *)(ws + lo.wtp[d]);
        bd.dgi = (float *)(ws + lo.dgi[d]);
        bd.dghn = (float *)(ws + lo.dghn[d]);
        bd.col0 = d * H;
        bd.reverse = d;
        // f16-split recurrence: bias sums per row group and the operand maxima come out of the kernel itself
        bd.bias_slab = r.fused_bias ? slabs + (size_t)d * n_rowgroups * 2 * H3 : nullptr;
        bd.mx_dgi = bwd_flag(c, lo) + enc_flag_dgi_max(l, d);
        bd.mx_dghn = bd.mx_dgi + 1;
    }
    if (ndir == 1)
        bp.dir[1] = bp.dir[0];
    if (top && c.sync && c.sync->wait_before_recurrence)
        TT_HIP_CHECK(hipStreamWaitEvent(st, (hipEvent_t)c.sync->wait_before_recurrence, 0));
    if (r.split_bwd) {
        // a row group's reduction over the gate columns on four CUs (gru16x4.hip); a time-out ORs bit 2 into `status`
        TT_RC_CHECK(gru16x4_bwd_launch(bp, ndir, ws + lo.xchb, c.status, st));
    } else if (r.use16) {
        TT_RC_CHECK(gru16_bwd_launch(bp, ndir, st));
    } else {
        const size_t lds = sizeof(float) * ENC_RB * (H3 + 4);
        TT_RC_CHECK(c.cell == CELL_LSTM ? launch_bwd_seq<CELL_LSTM>(bp, B, H, ndir, lds, st)
                                        : (c.cell == CELL_RNN ? launch_bwd_seq<CELL_RNN>(bp, B, H, ndir, lds, st)
                                                              : launch_bwd_seq<CELL_GRU>(bp, B, H, ndir, lds, st)));
    }
    if (l == 0 && c.sync && c.sync->record_after_recurrence)
        TT_HIP_CHECK(hipEventRecord((hipEvent_t)c.sync->record_after_recurrence, st));
    return TT_OK;
}

// bias sums, fused form: the recurrence kernel left one partial sum per row group in the split-K scratch: reduce them
// (row-group order: deterministic) for BOTH directions before the first weight-gradient product reuses that scratch
static int bwd_bias_reduce(const EncCall &c, const EncLayout &lo, int l)
{
    const int ndir = lo.ndir, H3 = lo.ng * c.H, n_rowgroups = (c.B + ENC_RB - 1) / ENC_RB;
    const float *slabs = (const float *)((char *)c.workspace + lo.slabs);
    for (int d = 0; d < ndir; ++d) {
        float *const *g = c.bwd->grads + ((size_t)l * ndir + d) * 4;
        hipLaunchKernelGGL(bias_reduce_kernel, dim3((2 * H3 + 31) / 32), dim3(256), 0, c.st, slabs + (size_t)d * n_rowgroups * 2 * H3,
                           n_rowgroups, H3, g[2], g[3]);
    }
    TT_LAUNCH_CHECK();
    return TT_OK;
}

// bias sums of one direction as column-sum passes: b_ih <- colsum(dGi); b_hh <- colsum(dGh) (GRU: the n gate's hidden-side
// pre-activation is scaled by r) or the same sums (LSTM / RNN: one pre-activation per gate).  The passes also find the maxima
// that scale the f16-split products behind them.
static int bwd_bias_colsums(const EncCall &c, const EncLayout &lo, int l, int d)
{
    char *ws = (char *)c.workspace;
    const SplitK k = bwd_splitk(c, lo);
    const int H3 = lo.ng * c.H;
    float *const *g = c.bwd->grads + ((size_t)l * lo.ndir + d) * 4;
    unsigned *mx = bwd_dg_max(c, lo, l, d);
    TT_RC_CHECK(colsum({(const float *)(ws + lo.dgi[d]), H3, k.MT, k.m_valid, g[2], mx}, k.slabs, k.st));
    if (c.cell == CELL_GRU)
        return colsum({(const float *)(ws + lo.dghn[d]), H3, k.MT, k.m_valid, g[3], mx ? mx + 1 : nullptr}, k.slabs, k.st);
    TT_HIP_CHECK(hipMemcpyAsync(g[3], g[2], sizeof(float) * H3, hipMemcpyDeviceToDevice, k.st));
    return TT_OK;
}

// the two weight-gradient products of layer l, direction d
static int bwd_weight_grads(const EncCall &c, const EncLayout &lo, const EncRoute &r, int l, int d)
{
    char *ws = (char *)c.workspace;
    const SplitK k = bwd_splitk(c, lo);
    const int H = c.H, ndir = lo.ndir, H3 = lo.ng * H, I = l == 0 ? c.E : ndir * H;
    const bool gru = c.cell == CELL_GRU;
    float *const *g = c.bwd->grads + ((size_t)l * ndir + d) * 4;
    const float *dgi = (const float *)(ws + lo.dgi[d]), *dghn = (const float *)(ws + lo.dghn[d]);
    const unsigned *mx_dgi = bwd_dg_max(c, lo, l, d), *mx_dghn = mx_dgi ? mx_dgi + 1 : nullptr;
    // W_ih <- dGi^T X   (X = gathered table rows for layer 0, the layer below's output above)
    // (f16-split products: embedding rows scaled by the power of two of the batch's largest |x|, which the training
    //  forward left in the status block; hidden states (|h| < 1, times 1/(1-p) when dropped) 2^6)
    if (l == 0)
        TT_RC_CHECK(gemm_tn({dgi, H3, H3, c.table, c.E, (const int32_t *)(ws + lo.ids), c.V, c.E, mx_dgi, 0,
                             bwd_flag(c, lo) + ENC_FLAG_XMAX, g[0]}, k));
    else
        TT_RC_CHECK(gemm_tn({dgi, H3, H3, (const float *)(ws + (r.drop ? lo.xd[l] : lo.x[l])), I, nullptr, k.MT, I, mx_dgi, 6, nullptr,
                             g[0]}, k));
    // W_hh <- dGh^T H_prev, H_prev rows through the previous-token map into this layer's own output
    // (GRU: the hidden-side gradients dGh = [dr_pre, dz_pre, dn_pre r]; LSTM / RNN: the same matrix as dGi)
    const float *hseq = (const float *)(ws + lo.x[l + 1]);
    return gemm_tn({gru ? dghn : dgi, H3, H3, hseq + (size_t)d * H, ndir * H, (const int32_t *)(ws + lo.prevmap[d]), (int64_t)k.MT + 1, H,
                    gru ? mx_dghn : mx_dgi, 10, nullptr, g[1]}, k);
}

// gradient w.r.t. layer l's input sequence, accumulated over the directions (below layer 0: w.r.t. the gathered vectors)
static int bwd_input_grad(const EncCall &c, const EncLayout &lo, int l, int d)
{
    char *ws = (char *)c.workspace;
    const SplitK k = bwd_splitk(c, lo);
    const int H3 = lo.ng * c.H, I = l == 0 ? c.E : lo.ndir * c.H;
    SgemmParams x;
    x.A = (const float *)(ws + lo.dgi[d]);
    x.B = c.weights[((size_t)l * lo.ndir + d) * 4];
    x.C = l > 0 ? (float *)(ws + lo.dx[l & 1]) : (float *)(ws + lo.dx0);
    x.m_dyn = k.m_valid;
    x.M = k.MT;
    x.N = I;
    x.K = H3;
    x.lda = H3;
    x.ldb = x.ldc = I;
    x.accumulate = d;
    if (c.o.force_f32)
        return tt_sgemm(x, false, true, 1, k.st);
    // on the f16 pipes like every other product of the step: dGi scaled by its maximum (the recurrence kernel or the
    // column-sum pass found it), W_ih by the power of two the forward pass derived
    x.a_absmax = bwd_dg_max(c, lo, l, d);
    x.b_absmax = bwd_flag(c, lo) + enc_flag_wih_max(l, d);
    return tt_sgemm16(x, false, true, 1, k.st);
}

// nn.Embedding backward (model.py:23-27 without GloVe vectors): row id accumulates the input gradients of the positions
// that hold it; padding_idx = 0 gets none.  Dense [V,E] gradient, as torch's.
static int bwd_table_scatter(const EncCall &c, const EncLayout &lo)
{
    char *ws = (char *)c.workspace;
    const SplitK k = bwd_splitk(c, lo);
    TT_RC_CHECK(tt_zero_async(c.bwd->g_table, sizeof(float) * (size_t)c.V * c.E, k.st));
    hipLaunchKernelGGL(table_scatter_kernel, dim3(2048), dim3(256), 0, k.st, (const float *)(ws + lo.dx0),
                       (const int32_t *)(ws + lo.ids), k.m_valid, k.MT, c.E, c.bwd->g_table);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_encoder_backward_f32(const int64_t *ids, int B, int T, const float *table, int64_t V, int E, int H,
                                      int num_layers, int bidirectional, int rnn_type, const float *const *weights,
                                      const float *proj_w, const float *proj_b, int normalize, float dropout_p,
                                      uint64_t dropout_seed, const float *d_out, float *const *grads,
                                      float *g_proj_w, float *g_proj_b, float *g_table, void *workspace,
                                      size_t workspace_bytes, int opts, int32_t *status, const tt_enc_sync_t *sync,
                                      tt_stream_t stream)
{
    const EncBwd b = {d_out, grads, g_proj_w, g_proj_b, g_table};
    // the record of the forward call that filled the workspace (train = 2 when the table is trained): opts must repeat its
    // TT_ENC_F32 and TT_ENC_SEED_ON_DEVICE, so that the route and the dropout masks are that call's
    const EncCall c = {{B, T, E, H, num_layers, bidirectional, rnn_type}, "tt_encoder_backward_f32", V, ids, table, weights, proj_w,
                       proj_b, /*prepared=*/nullptr, /*projected=*/nullptr, enc_opts(opts, g_table ? 2 : 1, dropout_seed),
                       dropout_p, normalize, /*out=*/nullptr, workspace, workspace_bytes, status, sync, (hipStream_t)stream, &b};
    EncLayout lo;
    TT_RC_CHECK(enc_validate(c, lo));
    const EncRoute r = enc_route(c, lo);
    TT_RC_CHECK(bwd_head(c, lo));
    for (int l = c.L - 1; l >= 0; --l) {
        TT_RC_CHECK(bwd_recurrence(c, lo, r, l));
        if (r.fused_bias)
            TT_RC_CHECK(bwd_bias_reduce(c, lo, l));
        for (int d = 0; d < lo.ndir; ++d) {
            if (!r.fused_bias)
                TT_RC_CHECK(bwd_bias_colsums(c, lo, l, d));
            TT_RC_CHECK(bwd_weight_grads(c, lo, r, l, d));
            if (l > 0 || g_table) // (below layer 0 only when the table is trained)
                TT_RC_CHECK(bwd_input_grad(c, lo, l, d));
        }
    }
    return g_table ? bwd_table_scatter(c, lo) : TT_OK;
}

