// Adam on the rows one call saw (edgegaussians_amd/optim.py: SparseAdam, SelectiveAdam).
//
// Two entries over ONE row update, adam_row1 -- adam1's style (csrc/project_dev.h): no contraction, separate multiplies
// and adds in a fixed order, the hardware's 1-ulp v_sqrt_f32 / v_rcp_f32 for the reasons given there:
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= step_size * m / (sqrt(v) + eps)
// eps is added to the UNCORRECTED root (torch/optim/_functional.py: sparse_adam; gsplat's selective_adam): the second
// bias correction sits in step_size = lr sqrt(1 - b2^t) / (1 - b1^t) (the index-list form; formed in double on the host
// and cast, as make_adamk does) or nowhere (the mask form: step_size = lr).  This is NOT adam1's
// sqrt(v) / sqrt(1 - b2^t) + eps, which is why the two do not share that function.
//
// eg_adam_sparse_rows: the gradient of a torch.sparse_coo_tensor with sparse_dim 1 -- values [nnz, w] and one row index
//   per value row.  The caller hands the indices SORTED (ascending) and the permutation that sorted them (a stable sort:
//   equal indices keep the order of the values tensor), or no permutation when the gradient is coalesced (the indices
//   are the tensor's own, strictly ascending).  One thread per (sorted position, component): a position whose
//   predecessor carries the same index does nothing; a position that STARTS a run walks the run through the
//   permutation, adds its values in fp32 first to last, and updates the row with the sum -- the inverted-index form of a
//   scatter-add: no float atomics, the same bits every run.  Rows that occur nowhere are not read and not written (their
//   moments do not decay); a row index outside [0, N) is skipped, so nothing outside the three tensors is ever written.
//   Skew: one thread walks a whole run, so a row that occurs thousands of times is summed serially while its
//   neighbours wait for nothing -- slow, correct, and not the shape the packed projection produces (a row occurs at most
//   once per camera).  The chunked form (partial sums per chunk, added in chunk order) is not built.
// eg_adam_masked_rows: dense gradient, rows of M components, stepped where visibility[row] != 0; every other row keeps
//   p, m and v bit for bit (not loaded, not stored).
#include "common.h"

namespace eg {

struct AdamRowK {
  float step_size, b1, omb1, b2, omb2, eps;
};

__device__ __forceinline__ void adam_row1(float &p, float g, float &m, float &v, const AdamRowK &h) {
#pragma clang fp contract(off)  // (one rounding sequence in both kernels)
  m = m * h.b1 + g * h.omb1;
  v = v * h.b2 + (g * g) * h.omb2;
  const float denom = __builtin_amdgcn_sqrtf(v) + h.eps;
  p = p - h.step_size * (m * __builtin_amdgcn_rcpf(denom));
}

__global__ void __launch_bounds__(256)
adam_sparse_rows_kernel(float *__restrict__ p, float *__restrict__ m, float *__restrict__ v,
                        const float *__restrict__ values, const long long *__restrict__ sorted_idx,
                        const long long *__restrict__ perm, unsigned total, unsigned nnz, long long N, unsigned w,
                        const AdamRowK h) {
#pragma clang fp contract(off)
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned pos = i / w, c = i - pos * w;
  const long long row = sorted_idx[pos];
  if (pos > 0 && sorted_idx[pos - 1] == row) return;  // (inside a run: its first position owns the row)
  if (row < 0 || row >= N) return;
  long long src = perm ? perm[pos] : (long long)pos;
  if (src < 0 || src >= (long long)nnz) return;       // (a permutation is a bijection of [0, nnz): anything else is not read)
  float g = values[(size_t)src * w + c];
  for (unsigned q = pos + 1; q < nnz && sorted_idx[q] == row; ++q) {
    src = perm ? perm[q] : (long long)q;
    if (src < 0 || src >= (long long)nnz) return;
    g = g + values[(size_t)src * w + c];
  }
  const size_t e = (size_t)row * w + c;
  float pp = p[e], mm = m[e], vv = v[e];
  adam_row1(pp, g, mm, vv, h);
  p[e] = pp; m[e] = mm; v[e] = vv;
}

__global__ void __launch_bounds__(256)
adam_masked_rows_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                        float *__restrict__ v, const uint8_t *__restrict__ visibility, unsigned total, unsigned M,
                        const AdamRowK h) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  if (!visibility[i / M]) return;
  float pp = p[i], mm = m[i], vv = v[i];
  adam_row1(pp, g[i], mm, vv, h);
  p[i] = pp; m[i] = mm; v[i] = vv;
}

static AdamRowK make_adam_rowk(double step_size, double beta1, double beta2, double eps) {
  AdamRowK k;
  k.step_size = (float)step_size;
  k.b1 = (float)beta1; k.omb1 = (float)(1.0 - beta1);
  k.b2 = (float)beta2; k.omb2 = (float)(1.0 - beta2);
  k.eps = (float)eps;
  return k;
}

}  // namespace eg

using namespace eg;

extern "C" int eg_adam_sparse_rows(float *param, float *exp_avg, float *exp_avg_sq, const float *values,
                                   const int64_t *sorted_indices, const int64_t *perm, int64_t nnz, int64_t N, int32_t w,
                                   double lr, double beta1, double beta2, double eps, int32_t step,
                                   eg_stream_t stream) {
  EG_REQUIRE(nnz >= 0 && N >= 0, "negative size (nnz, N)");
  EG_REQUIRE(w >= 1, "w (the row width) must be at least 1");
  EG_REQUIRE(step >= 1, "step is 1-based");
  EG_REQUIRE(nnz < (1ll << 31) / w, "nnz * w must be below 2^31");
  if (nnz == 0 || N == 0) return EG_OK;
  EG_REQUIRE(param, "param is null");
  EG_REQUIRE(exp_avg, "exp_avg is null");
  EG_REQUIRE(exp_avg_sq, "exp_avg_sq is null");
  EG_REQUIRE(values, "values is null");
  EG_REQUIRE(sorted_indices, "sorted_indices is null");
  const double t = (double)step;
  const double step_size = lr * sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t));
  const unsigned total = (unsigned)(nnz * w);
  adam_sparse_rows_kernel<<<cdiv(total, 256), 256, 0, as_stream(stream)>>>(
      param, exp_avg, exp_avg_sq, values, (const long long *)sorted_indices, (const long long *)perm, total,
      (unsigned)nnz, (long long)N, (unsigned)w, make_adam_rowk(step_size, beta1, beta2, eps));
  return check_launch("adam_sparse_rows");
}

extern "C" int eg_adam_masked_rows(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                                   const uint8_t *visibility, int64_t N, int32_t M, double lr, double beta1,
                                   double beta2, double eps, eg_stream_t stream) {
  EG_REQUIRE(N >= 0, "negative size (N)");
  EG_REQUIRE(M >= 1, "M (the row width) must be at least 1");
  EG_REQUIRE(N < (1ll << 31) / M, "N * M must be below 2^31");
  if (N == 0) return EG_OK;
  EG_REQUIRE(param, "param is null");
  EG_REQUIRE(grad, "grad is null");
  EG_REQUIRE(exp_avg, "exp_avg is null");
  EG_REQUIRE(exp_avg_sq, "exp_avg_sq is null");
  EG_REQUIRE(visibility, "visibility is null");
  const unsigned total = (unsigned)(N * M);
  adam_masked_rows_kernel<<<cdiv(total, 256), 256, 0, as_stream(stream)>>>(
      param, grad, exp_avg, exp_avg_sq, visibility, total, (unsigned)M, make_adam_rowk(lr, beta1, beta2, eps));
  return check_launch("adam_masked_rows");
}
