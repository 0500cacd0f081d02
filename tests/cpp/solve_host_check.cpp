// solve_host_check.cpp -- the two pieces of icpslam_amd/csrc/icp_solver.cpp that the library does not export, driven from stdin, one request
// per line, every double as the 16 hex digits of its bits (nothing is rounded on the way in or out).  tests/test_solve_host.py builds it
// from icp_solver.cpp alone and runs it.
//   svd  a00 a01 .. a22                         -> U (9, row-major)  s (3)  V (9), as hex words
//   conv max_iterations transformation_epsilon euclidean_fitness_epsilon force n  then n times  nr_iterations r00 r11 r22 tx ty tz mse
//                                               -> n times "returned:state" from ONE ConvergenceCriteria, in call order
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "icp_solver.h"

static bool get(std::istream& in, double& x) {
  std::string w;
  if (!(in >> w)) return false;
  const uint64_t bits = std::strtoull(w.c_str(), nullptr, 16);
  std::memcpy(&x, &bits, sizeof(x));
  return true;
}

static void put(double x) {
  uint64_t bits;
  std::memcpy(&bits, &x, sizeof(x));
  std::printf(" %016" PRIx64, bits);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "svd") {
      double A[9], U[9], s[3], V[9];
      for (double& a : A)
        if (!get(in, a)) return 2;
      icpgpu::svd3x3(A, U, s, V);
      std::printf("svd");
      for (double x : U) put(x);
      for (double x : s) put(x);
      for (double x : V) put(x);
      std::printf("\n");
    } else if (what == "conv") {
      int max_iterations, force, n;
      double teps, feps;
      if (!(in >> max_iterations) || !get(in, teps) || !get(in, feps) || !(in >> force >> n)) return 2;
      icpgpu::ConvergenceCriteria crit(max_iterations, teps, feps, force != 0);
      std::printf("conv");
      for (int k = 0; k < n; ++k) {
        int nr;
        double v[7];
        if (!(in >> nr)) return 2;
        for (double& x : v)
          if (!get(in, x)) return 2;
        icpgpu::Mat4d Tk = icpgpu::mat4_identity();
        Tk[0] = v[0], Tk[5] = v[1], Tk[10] = v[2], Tk[12] = v[3], Tk[13] = v[4], Tk[14] = v[5];
        const bool stop = crit.has_converged(nr, Tk, v[6]);
        std::printf(" %d:%d", stop ? 1 : 0, crit.state());
      }
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
