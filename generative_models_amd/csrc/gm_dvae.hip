// Denoising VAE (dvae.py; gm_hip.h; the rule in gm_dvae.h).
//
// gm_dvae_corrupt: one thread per pixel quad of a row (one Philox call -> the four pixels), rows ldx / ldo floats apart;
//   16-byte loads and stores where the rows allow them, element by element otherwise.  What dvae.corrupt() and the
//   general path's compute_batch run.
// gm_gather_rows_corrupt[_bits]: gm_gather_rows[_bits] that also writes the corrupted copy of every gathered row (one
//   row per wave, 4 waves per workgroup; gather_corrupt_body).  The engine's first batch of a graph; the others get
//   theirs from the corrupting gather riding in the [mu | log_var] forward (ops_fused.linear_fwd_gather_corrupt, gm_gemm.hip).
// No atomics, no reductions: the same bits on every run.
#include "gm_dvae.h"

namespace {

struct CorruptRowsP {
    const float* x; int64_t ldx;
    float* out; int64_t ldo;
    int64_t rows; int row_elems, nq, vec;
};

__global__ __launch_bounds__(256) void dvae_corrupt_kernel(CorruptRowsP p, CorruptP c) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= p.rows * p.nq) return;
    const int64_t r = gi / p.nq;
    const int q = (int)(gi - r * p.nq);
    const uint32_t step = ph_step(c.clk), row = (uint32_t)(c.row0 + r);
    const float* xs = p.x + r * p.ldx;
    float* o = p.out + r * p.ldo;
    if (p.vec) {
        const float4 v = reinterpret_cast<const float4*>(xs)[q];
        reinterpret_cast<float4*>(o)[q] = corrupt4(c, step, row, (uint32_t)q, v);
        return;
    }
    const int n = min(4, p.row_elems - 4 * q);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    v.x = xs[4 * q];
    if (n > 1) v.y = xs[4 * q + 1];
    if (n > 2) v.z = xs[4 * q + 2];
    if (n > 3) v.w = xs[4 * q + 3];
    const float4 y = corrupt4(c, step, row, (uint32_t)q, v);
    for (int j = 0; j < n; ++j) o[4 * q + j] = ph_lane(y, j);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int gm_dvae_corrupt(void* stream, const gm_corrupt_args* a, const float* x, int64_t ldx, float* out,
                               int64_t ldo, int64_t rows, int row_elems) {
    CorruptP c{};
    const int rc = gm_corrupt_fill(a, &c);
    if (rc) return rc;
    GM_CHECK_ARG(x && out && rows >= 0 && row_elems > 0 && ldx >= row_elems && ldo >= row_elems);
    GM_CHECK_ARG((const float*)out != x || ldx == ldo);       // in place: row by row, each quad read then written
    const int nq = (row_elems + 3) / 4;
    GM_CHECK_ARG(rows < (1ll << 40) / nq);
    if (rows == 0) return 0;
    CorruptRowsP p{x, ldx, out, ldo, rows, row_elems, nq,
                   (row_elems % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && al16(x) && al16(out)) ? 1 : 0};
    const int64_t blocks = (rows * nq + 255) / 256;
    GM_CHECK_ARG(blocks < (1ll << 31));
    hipLaunchKernelGGL(dvae_corrupt_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, c);
    GM_LAUNCH_RET();
}

extern "C" int gm_gather_rows_corrupt(void* stream, const gm_corrupt_args* a, const float* data, int64_t n_rows,
                                      const int64_t* idx, gm_slot idx_slot, float* out, float* out_c, int64_t ld_out,
                                      int B, int row_elems) {
    GatherP g{};
    CorruptP c{};
    int rc = gm_gather_fill(data, n_rows, idx, idx_slot, out, ld_out, B, row_elems, &g);
    if (rc) return rc;
    rc = gm_gather_corrupt_fill(a, out_c, &g, &c);
    if (rc) return rc;
    hipLaunchKernelGGL(gather_rows_corrupt_kernel, dim3(gm_gather_blocks(g, 4)), dim3(256), 0, (hipStream_t)stream, g,
                       c);
    GM_LAUNCH_RET();
}

extern "C" int gm_gather_rows_bits_corrupt(void* stream, const gm_corrupt_args* a, const uint32_t* bits,
                                           int words_per_row, int64_t n_rows, const int64_t* idx, gm_slot idx_slot,
                                           float* out, float* out_c, int64_t ld_out, int B, int row_elems) {
    GatherP g{};
    CorruptP c{};
    int rc = gm_gather_fill_bits(bits, words_per_row, n_rows, idx, idx_slot, out, ld_out, B, row_elems, &g);
    if (rc) return rc;
    rc = gm_gather_corrupt_fill(a, out_c, &g, &c);
    if (rc) return rc;
    hipLaunchKernelGGL(gather_rows_corrupt_kernel, dim3(gm_gather_blocks(g, 4)), dim3(256), 0, (hipStream_t)stream, g,
                       c);
    GM_LAUNCH_RET();
}
