// mls_host_check.cpp -- the moving least squares' shared definitions on the host: icpslam_amd/csrc/icp_exp.h (exp_neg), icp_jacobi3.h
// and icp_mls.h (mls_plane, mls_solve), the very functions the kernels of icp_mls.hip call, driven over given neighbour rows with the
// rule's 64-partial sums written out as a loop.  tests/test_mls_host.py builds it (host only), feeds it the hand cases' rows and
// compares what it writes with tests/mls_restated.py, bit for bit; built with -fsanitize=address,undefined it is the stand-alone
// program that checks this code for memory errors and undefined behaviour.
//   mls_host_check exp                 reads doubles from stdin (hex words), prints exp_neg of each as a hex word
//   mls_host_check rows IN OUT         IN: int32 n, n_q, order, total; double s; cloud (n float4); queries (n_q float4); row_start
//                                      (n_q + 1 int32); idx (total int32).  OUT: status (n_q int32), plane7 (n_q x 7 double), coeff10
//                                      (n_q x 10 double), points (n_q float4), normals (n_q float4) -- per query, not compacted
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "icp_exp.h"
#include "icp_mls.h"

namespace {

// WSUM over a row: term(t, out) fills the S terms of entry t
template <int S, class F>
void wsum(int m, double (&sum)[S], F&& term) {
  std::vector<double> part(64 * S, 0.0);
  double v[S];
  for (int t = 0; t < m; ++t) {
    term(t, v);
    for (int e = 0; e < S; ++e) part[(t & 63) * S + e] = part[(t & 63) * S + e] + v[e];
  }
  std::vector<double> next(64 * S);
  for (int mask = 32; mask > 0; mask >>= 1) {
    for (int l = 0; l < 64; ++l)
      for (int e = 0; e < S; ++e) next[l * S + e] = part[l * S + e] + part[(l ^ mask) * S + e];
    part.swap(next);
  }
  for (int e = 0; e < S; ++e) sum[e] = part[e];
}

template <int ORDER>
int fit(const float* cloud, const int32_t* row, int m, const icpgpu::MlsPlane& pl, double s, double* coeff, double (&point)[3], double (&normal)[3]) {
  constexpr int NC = icpgpu::mls_coefficients(ORDER), NA = NC * (NC + 1) / 2, NS = icpgpu::mls_sums(ORDER);
  double sums[NS];
  wsum<NS>(m, sums, [&](int t, double (&v)[NS]) {
    const float* q = cloud + 4 * (size_t)row[t];
    const double dx = (double)q[0] - pl.Q[0], dy = (double)q[1] - pl.Q[1], dz = (double)q[2] - pl.Q[2];
    const double dd = (dx * dx + dy * dy) + dz * dz;
    const double w = icpgpu::exp_neg(-dd / s);
    const double u = (dx * pl.U[0] + dy * pl.U[1]) + dz * pl.U[2];
    const double vv = (dx * pl.V[0] + dy * pl.V[1]) + dz * pl.V[2];
    const double f = (dx * pl.N[0] + dy * pl.N[1]) + dz * pl.N[2];
    double P[NC];
    int j = 0;
    double u_pow = 1.0;
    for (int ui = 0; ui <= ORDER; ++ui) {
      double v_pow = 1.0;
      for (int vi = 0; vi <= ORDER - ui; ++vi) {
        P[j++] = u_pow * v_pow;
        v_pow = v_pow * vv;
      }
      u_pow = u_pow * u;
    }
    for (int a = 0; a < NC; ++a) {
      const double pw = P[a] * w;
      for (int b = 0; b <= a; ++b) v[a * (a + 1) / 2 + b] = pw * P[b];
      v[NA + a] = pw * f;
    }
  });
  double A[NA], c[NC];
  for (int e = 0; e < NA; ++e) A[e] = sums[e];
  for (int e = 0; e < NC; ++e) c[e] = sums[NA + e];
  icpgpu::mls_solve<NC>(A, c);
  for (int e = 0; e < NC; ++e) coeff[e] = c[e];
  if (!std::isfinite(c[0])) return 3;
  for (int e = 0; e < 3; ++e) {
    point[e] = pl.Q[e] + c[0] * pl.N[e];
    normal[e] = (pl.N[e] - c[ORDER + 1] * pl.U[e]) - c[1] * pl.V[e];
  }
  return 2;
}

template <class T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int run_rows(const char* in_path, const char* out_path) {
  FILE* f = fopen(in_path, "rb");
  if (!f) return 2;
  int32_t head[4];
  double s;
  if (fread(head, sizeof head, 1, f) != 1 || fread(&s, sizeof s, 1, f) != 1) return 2;
  const int n = head[0], n_q = head[1], order = head[2], total = head[3];
  std::vector<float> cloud, queries;
  std::vector<int32_t> row_start, idx;
  if (!read_n(f, cloud, (size_t)n * 4) || !read_n(f, queries, (size_t)n_q * 4) || !read_n(f, row_start, (size_t)n_q + 1) || !read_n(f, idx, (size_t)total))
    return 2;
  fclose(f);
  const double nan = __builtin_nan("");
  const float nanf_ = __builtin_nanf("");
  std::vector<int32_t> status(n_q, 0);
  std::vector<double> plane7((size_t)n_q * 7, nan), coeff10((size_t)n_q * 10, nan);
  std::vector<float> points((size_t)n_q * 4, nanf_), normals((size_t)n_q * 4, nanf_);
  for (int i = 0; i < n_q; ++i) {
    const int32_t* row = idx.data() + row_start[i];
    const int m = row_start[i + 1] - row_start[i];
    if (m < 3) continue;
    const float* k4 = cloud.data() + 4 * (size_t)row[0];
    const double K[3] = {(double)k4[0], (double)k4[1], (double)k4[2]};
    const double P[3] = {(double)queries[4 * (size_t)i], (double)queries[4 * (size_t)i + 1], (double)queries[4 * (size_t)i + 2]};
    double sums[9];
    wsum<9>(m, sums, [&](int t, double (&v)[9]) {
      const float* q = cloud.data() + 4 * (size_t)row[t];
      const double dx = (double)q[0] - K[0], dy = (double)q[1] - K[1], dz = (double)q[2] - K[2];
      v[0] = dx * dx, v[1] = dx * dy, v[2] = dx * dz, v[3] = dy * dy, v[4] = dy * dz, v[5] = dz * dz, v[6] = dx, v[7] = dy, v[8] = dz;
    });
    icpgpu::MlsPlane pl;
    icpgpu::mls_plane(sums, m, K, P, pl);
    for (int e = 0; e < 3; ++e) plane7[(size_t)i * 7 + e] = pl.N[e], plane7[(size_t)i * 7 + 3 + e] = pl.c[e];
    plane7[(size_t)i * 7 + 6] = pl.lambda;
    double point[3] = {pl.Q[0], pl.Q[1], pl.Q[2]}, normal[3] = {pl.N[0], pl.N[1], pl.N[2]};
    status[i] = 1;
    if (order == 2 && m >= 6) status[i] = fit<2>(cloud.data(), row, m, pl, s, &coeff10[(size_t)i * 10], point, normal);
    if (order == 3 && m >= 10) status[i] = fit<3>(cloud.data(), row, m, pl, s, &coeff10[(size_t)i * 10], point, normal);
    for (int e = 0; e < 3; ++e) points[(size_t)i * 4 + e] = (float)point[e], normals[(size_t)i * 4 + e] = (float)normal[e];
    points[(size_t)i * 4 + 3] = 1.f;
    normals[(size_t)i * 4 + 3] = pl.curvature;
  }
  FILE* o = fopen(out_path, "wb");
  if (!o) return 2;
  fwrite(status.data(), sizeof(int32_t), status.size(), o);
  fwrite(plane7.data(), sizeof(double), plane7.size(), o);
  fwrite(coeff10.data(), sizeof(double), coeff10.size(), o);
  fwrite(points.data(), sizeof(float), points.size(), o);
  fwrite(normals.data(), sizeof(float), normals.size(), o);
  fclose(o);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "exp")) {
    uint64_t bits;
    while (scanf("%" SCNx64, &bits) == 1) {
      double a, w;
      memcpy(&a, &bits, sizeof a);
      w = icpgpu::exp_neg(a);
      memcpy(&bits, &w, sizeof w);
      printf("%016" PRIx64 "\n", bits);
    }
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "rows")) return run_rows(argv[2], argv[3]);
  fprintf(stderr, "usage: mls_host_check exp | rows IN OUT\n");
  return 1;
}
