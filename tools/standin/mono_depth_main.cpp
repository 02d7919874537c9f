// Stand-alone host program: csrc/mono_depth.hip compiled for the CPU against the shim of the HIP names in this folder
// (256 real threads per workgroup, a barrier for __syncthreads), for AddressSanitizer and UBSan.  Every case file
// (mono_depth_cases.py writes them from tests/mono_depth_reference.py) must give the float64 restatement's losses and
// gradients within 4 * 2^-24 (losses relative, gradients relative to the largest entry), the same NaN pattern, and
// untouched guard bands around every output.
//   python tools/standin/mono_depth_cases.py DIR && clang++ -std=c++20 -O1 -g -fsanitize=address,undefined \
//     -x c++ -Itools/standin -Igaussian-splatting-toolkit_amd/csrc -include hip/hip_runtime.h \
//     tools/standin/mono_depth_main.cpp -o DIR/mono_depth_standin -lpthread && DIR/mono_depth_standin DIR/*.bin
#include <cstdarg>
#include "mono_depth.hip"
static char last_error[512];
void gsr_set_error(const char *fmt, ...) { va_list a; va_start(a, fmt); vsnprintf(last_error, sizeof last_error, fmt, a); va_end(a); }
static const double TOL = 4.0 / 16777216.0;
static const int GUARD = 64;
static bool close_loss(float got, double want) { return std::isnan(want) ? std::isnan(got) : std::fabs((double)got - want) <= TOL * std::fabs(want); }
// gradient [n] inside guard bands of GUARD floats of -7
static bool close_grad(const std::vector<float> &v, const std::vector<double> &want, const char *what) {
  const size_t n = want.size();
  double top = 0.0, worst = 0.0;
  bool ok = true;
  for (size_t i = 0; i < n; ++i) if (!std::isnan(want[i])) top = std::max(top, std::fabs(want[i]));
  for (size_t i = 0; i < n; ++i) {
    const float g = v[GUARD + i];
    if (std::isnan(want[i]) != std::isnan(g)) ok = false;
    else if (!std::isnan(g)) worst = std::max(worst, std::fabs((double)g - want[i]));
  }
  ok = ok && worst <= TOL * (top > 0 ? top : 1.0);
  for (int i = 0; i < GUARD; ++i) ok = ok && v[i] == -7.f && v[GUARD + n + i] == -7.f;
  if (!ok) printf("  %s gradient differs (worst %.3g of %.3g)\n", what, worst, top);
  return ok;
}
template <class T> static bool get(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
int main(int argc, char **argv) {
  int failed = 0, ran = 0;
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb");
    int hd[6];  // H, W, box, n_corr, idx64, masked
    float ss[2];
    if (!f || fread(hd, 4, 6, f) != 6 || fread(ss, 4, 2, f) != 2) { printf("%s: unreadable\n", argv[a]); return 2; }
    const int H = hd[0], W = hd[1], box = hd[2], nc = hd[3], idx64 = hd[4], masked = hd[5];
    const size_t n = (size_t)H * W;
    std::vector<float> pred(n), gt(n), img(3 * n), mask(masked ? n : 0);
    std::vector<char> rows((size_t)nc * (idx64 ? 8 : 4)), cols(rows.size());
    std::vector<double> want(3), g0(n), g1(n), g2(n);
    if (!get(f, pred) || !get(f, gt) || !get(f, img) || !get(f, mask) || !get(f, rows) || !get(f, cols) || !get(f, want) ||
        !get(f, g0) || !get(f, g1) || !get(f, g2)) { printf("%s: short\n", argv[a]); return 2; }
    fclose(f);
    const float *m = masked ? mask.data() : nullptr;
    // (exactly-sized heap blocks: an access one element past any of them is an AddressSanitizer report)
    std::vector<double> stats((size_t)std::max(nc, 1) * 5, -7.0), partial(GSR_MONO_DEPTH_WORKSPACE_DOUBLES, -7.0);
    const float up = -2.5f;
    for (auto *g : {&g0, &g1, &g2}) for (double &v : *g) v *= (double)up;
    float loss[3] = {-7.f, -7.f, -7.f};
    std::vector<float> v0(n + 2 * GUARD, -7.f), v1(v0), v2(v0);
    bool ok = true;
    int rc = gsr_local_pearson_forward(H, W, box, nc, pred.data(), gt.data(), m, rows.data(), cols.data(), idx64, stats.data(), &loss[0], nullptr);
    rc = rc ? rc : gsr_local_pearson_backward(H, W, box, nc, &up, pred.data(), gt.data(), m, rows.data(), cols.data(), idx64, stats.data(), v0.data() + GUARD, nullptr);
    rc = rc ? rc : gsr_log_depth_forward(H, W, pred.data(), gt.data(), img.data(), ss, m, partial.data(), &loss[1], nullptr);
    rc = rc ? rc : gsr_log_depth_backward(H, W, &up, pred.data(), gt.data(), img.data(), ss, m, v1.data() + GUARD, nullptr);
    rc = rc ? rc : gsr_tv_forward(H, W, pred.data(), m, partial.data(), &loss[2], nullptr);
    rc = rc ? rc : gsr_tv_backward(H, W, &up, pred.data(), m, v2.data() + GUARD, nullptr);
    if (rc) { ok = false; printf("  rc %d (%s)\n", rc, last_error); }
    for (int k = 0; k < 3 && ok; ++k)
      if (!close_loss(loss[k], want[k])) { ok = false; printf("  loss %d: %.9g, want %.12g\n", k, loss[k], want[k]); }
    ok = ok && close_grad(v0, g0, "local Pearson") && close_grad(v1, g1, "log-depth") && close_grad(v2, g2, "TV");
    // argument checks: a box outside [1, min(H, W)] is refused before anything is launched
    ok = ok && gsr_local_pearson_forward(H, W, 0, nc, pred.data(), gt.data(), m, rows.data(), cols.data(), idx64, stats.data(), &loss[0], nullptr) == GSR_EINVAL;
    ok = ok && gsr_local_pearson_backward(H, W, std::min(H, W) + 1, nc, &up, pred.data(), gt.data(), m, rows.data(), cols.data(), idx64, stats.data(), v0.data() + GUARD, nullptr) == GSR_EINVAL;
    ++ran; failed += !ok;
    printf("%s H=%d W=%d box=%d patches=%d idx64=%d masked=%d losses %.7g %.7g %.7g: %s\n", argv[a], H, W, box, nc, idx64, masked, loss[0], loss[1], loss[2], ok ? "ok" : "FAILED");
  }
  printf("%d cases, %d failed\n", ran, failed);
  return failed != 0;
}
