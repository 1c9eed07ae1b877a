// cert.hpp -- the split scores and their certificate, shared by the kernels that score on the
// fp16 / bf16 planes (exact.hip, range.hip, part_scan.hip): one formula for a pair's score, one
// for the score threshold that covers a distance radius.
#pragma once
#include "device_common.hpp"
#include "engine.hpp"

namespace mh {

// Split-operand GEMM modes (planes of A = queries, B = rows, all K-blocked by 16):
//   RING_X3 bf16x3     q.x ~ ql.xh + qh.xl + qh.xh  (A hi+lo, B hi+lo)
//   RING_H2 fp16 2-pr. q.x ~ ql.xh + qh.xh          (A hi+lo, B hi; rows rounded once)
//   RING_H1 fp16 1-pr. q.x ~ qh.xh                  (A hi,    B hi; both rounded once)
enum { RING_X3 = 0, RING_H2 = 1, RING_H1 = 2 };

// the score of one (query, row) pair from its accumulator -- the one formula
// every consumer of split scores uses (write epilogue, candidate select), so
// a score is the same float wherever it is computed.  Outside the fp16 bound
// (NaN unscale): -inf, always preselected / never certified.
__device__ __forceinline__ float split_score(int mode, int metric, float acc, float xi, float qi, float qn, float xn) {
    const float dot = mode != RING_X3 ? acc * xi * qi : acc;
    float sc = metric == COSINE ? 1.0f - dot / (qn * xn) : fmaf(-2.f, dot, qn * qn + xn * xn);
    if (!(sc == sc)) sc = __int_as_float(0x7f800000);
    if (mode != RING_X3 && !(xi == xi && qi == qi)) sc = -__int_as_float(0x7f800000);
    return sc;
}

// k_rerank's certificate read the other way: the score threshold t of a distance radius r, rounded
// up -- a row whose canonical distance is <= r scores <= t (inclusive on both sides).  qn: the
// query's canonical norm; c: eps_cos / eps_dot / c_l2 / xmax / xerr / qerr.  NaN: no finite
// threshold covers the radius.
__device__ __forceinline__ float cert_score_thr(int metric, float r, float qn, const CertArgs& c) {
    const double xe = c.xerr ? (double)*c.xerr : 0.0, qe = c.qerr ? (double)*c.qerr : 0.0;
    double td;
    if (metric == COSINE) {
        // k_rerank: |score - d| <= eps_cos + ex
        const double ex = 1.01 * (1.0 + 1e-4) * (xe + qe + xe * qe);
        td = (double)r + (double)c.eps_cos + ex;
    } else {
        // k_rerank: |score - d^2| <= delta(q); d = sqrtf(s) <= r only if s <= r^2 (1 + 2^-23 + ..)
        const double qnd = qn, xm = *c.xmax;
        const double ed = c.eps_dot + 1.01 * (xe + qe + xe * qe);
        const double delta = 2.0 * ed * qnd * xm + c.c_l2 * (qnd + xm) * (qnd + xm);
        td = (double)r * (double)r * (1.0 + 0x1p-22) + delta;
    }
    float t = (float)td;
    if ((double)t < td)  // round up
        t = t > 0.f ? __uint_as_float(__float_as_uint(t) + 1u) : t < 0.f ? __uint_as_float(__float_as_uint(t) - 1u) : 1e-45f;
    return isfinite(t) ? t : __int_as_float(0x7fc00000);
}

}  // namespace mh
