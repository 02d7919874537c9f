// Stand-alone host program: csrc/bilagrid.hip compiled for the CPU against the shim of the HIP names in this folder
// (256 real threads per workgroup, a barrier for __syncthreads), for AddressSanitizer and UBSan.  Every case file
// (bilagrid_cases.py writes them from tests/_bilagrid_ref.py) must give the float64 restatement's outputs and
// gradients within 4 x the float32 restatement's error + 2^-23 (relative to the largest entry, the rule of
// tests/test_gpu_bilagrid.py), exact zeros for the views not sliced, the same bits from a second run, and untouched
// guard bands around every output.
//   python tools/standin/bilagrid_cases.py DIR && clang++ -std=c++20 -O1 -g -fsanitize=address,undefined \
//     -x c++ -Itools/standin -Igaussian-splatting-toolkit_amd/csrc -include hip/hip_runtime.h \
//     tools/standin/bilagrid_main.cpp -o DIR/bilagrid_standin -lpthread && DIR/bilagrid_standin DIR/*.bin
#include <cstdarg>
inline float __fdiv_rn(float a, float b) { return a / b; }
inline float __fadd_rn(float a, float b) { return a + b; }
inline float __fmul_rn(float a, float b) { return a * b; }
#include "bilagrid.hip"
static char last_error[512];
void gsr_set_error(const char *fmt, ...) { va_list a; va_start(a, fmt); vsnprintf(last_error, sizeof last_error, fmt, a); va_end(a); }
static const int GUARD = 64;
static const double ULP = 1.0 / 8388608.0;
// v [n] inside guard bands of GUARD floats of -7 against want: e = max |v - want| / max |want| <= 4 e32 + 2^-23
static bool close_to(const std::vector<float> &v, const std::vector<double> &want, double e32, const char *what) {
  const size_t n = want.size();
  double top = 0.0, worst = 0.0;
  for (size_t i = 0; i < n; ++i) top = std::max(top, std::fabs(want[i]));
  for (size_t i = 0; i < n; ++i) worst = std::max(worst, std::fabs((double)v[GUARD + i] - want[i]));
  const double e = worst / (top > 0 ? top : 1.0);
  bool ok = e <= 4.0 * e32 + ULP;
  for (int i = 0; i < GUARD; ++i) ok = ok && v[i] == -7.f && v[GUARD + n + i] == -7.f;
  printf("  %-8s e %.3g (float32 restatement %.3g, bound %.3g)%s\n", what, e, e32, 4.0 * e32 + ULP, ok ? "" : "  <-- FAILED");
  return ok;
}
template <class T> static bool get(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
int main(int argc, char **argv) {
  int failed = 0, ran = 0;
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb");
    int hd[7];  // H, W, V, view, Gw, Gh, L
    if (!f || fread(hd, 4, 7, f) != 7) { printf("%s: unreadable\n", argv[a]); return 2; }
    const int H = hd[0], W = hd[1], V = hd[2], view = hd[3], gw = hd[4], gh = hd[5], gl = hd[6];
    const size_t n = (size_t)H * W * 3, per = (size_t)gl * gh * gw * 12, ng = per * V;
    std::vector<float> rgb(n), v_out(n);
    // (aligned_alloc: the kernels read a vertex as three 16-byte loads)
    float *grids = (float *)aligned_alloc(16, (ng * 4 + 15) / 16 * 16);
    std::vector<double> w_out(n), w_rgb(n), w_grids(ng), w_tv(1), w_vtv(ng), e32(5);
    if (fread(grids, 4, ng, f) != ng || !get(f, rgb) || !get(f, v_out) || !get(f, w_out) || !get(f, w_rgb) || !get(f, w_grids) ||
        !get(f, w_tv) || !get(f, w_vtv) || !get(f, e32)) { printf("%s: short\n", argv[a]); return 2; }
    fclose(f);
    printf("%s H=%d W=%d V=%d view=%d grid %dx%dx%d\n", argv[a], H, W, V, view, gw, gh, gl);
    // (exactly-sized heap blocks: an access one element past any of them is an AddressSanitizer report)
    std::vector<double> work(GSR_BILAGRID_WORKSPACE_DOUBLES(gw, gh, gl), -7.0), partial(GSR_BILAGRID_TV_WORKSPACE_DOUBLES, -7.0);
    bool ok = true;
    std::vector<float> keep[3];
    for (int run = 0; run < 2 && ok; ++run) {
      std::vector<float> out(n + 2 * GUARD, -7.f), v_rgb(out), v_grids(ng + 2 * GUARD, -7.f), tv(1 + 2 * GUARD, -7.f), v_tv(v_grids);
      const float up = 1.f;
      std::fill(work.begin(), work.end(), run ? 1e300 : -7.0);  // (the workspace needs no zeroing)
      int rc = gsr_bilagrid_slice_forward(H, W, V, view, gw, gh, gl, grids, rgb.data(), out.data() + GUARD, nullptr);
      rc = rc ? rc : gsr_bilagrid_slice_backward(H, W, V, view, gw, gh, gl, grids, rgb.data(), v_out.data(), work.data(), v_rgb.data() + GUARD, v_grids.data() + GUARD, nullptr);
      rc = rc ? rc : gsr_bilagrid_tv_forward(V, gw, gh, gl, grids, partial.data(), tv.data() + GUARD, nullptr);
      rc = rc ? rc : gsr_bilagrid_tv_backward(V, gw, gh, gl, &up, grids, v_tv.data() + GUARD, nullptr);
      if (rc) { ok = false; printf("  rc %d (%s)\n", rc, last_error); break; }
      if (run == 0) {
        ok = close_to(out, w_out, e32[0], "out") & close_to(v_rgb, w_rgb, e32[1], "v_rgb") & close_to(v_grids, w_grids, e32[2], "v_grids") &
             close_to(tv, w_tv, e32[3], "tv") & close_to(v_tv, w_vtv, e32[4], "v_tv");
        for (int v = 0; v < V; ++v)
          if (v != view)
            for (size_t i = 0; i < per; ++i)
              if (v_grids[GUARD + v * per + i] != 0.f || std::signbit(v_grids[GUARD + v * per + i])) { ok = false; printf("  view %d not zero\n", v); break; }
        keep[0] = out, keep[1] = v_rgb, keep[2] = v_grids;
      } else if (memcmp(keep[0].data(), out.data(), out.size() * 4) || memcmp(keep[1].data(), v_rgb.data(), v_rgb.size() * 4) ||
                 memcmp(keep[2].data(), v_grids.data(), v_grids.size() * 4)) {
        ok = false, printf("  the second run differs\n");
      }
    }
    // argument checks: refused before anything is launched
    ok = ok && gsr_bilagrid_slice_forward(H, W, V, V, gw, gh, gl, grids, rgb.data(), nullptr, nullptr) == GSR_EINVAL;
    ok = ok && gsr_bilagrid_slice_forward(H, W, V, -1, gw, gh, gl, grids, rgb.data(), nullptr, nullptr) == GSR_EINVAL;
    ok = ok && gsr_bilagrid_tv_forward(V, 1, gh, gl, grids, partial.data(), nullptr, nullptr) == GSR_EINVAL;
    ok = ok && gsr_bilagrid_tv_forward(V, gw, 65, gl, grids, partial.data(), nullptr, nullptr) == GSR_EINVAL;
    ok = ok && gsr_bilagrid_tv_backward(V, gw, gh, 17, nullptr, grids, nullptr, nullptr) == GSR_EINVAL;
    free(grids);
    ++ran; failed += !ok;
    printf("  %s\n", ok ? "ok" : "FAILED");
  }
  printf("%d cases, %d failed\n", ran, failed);
  return failed != 0;
}
