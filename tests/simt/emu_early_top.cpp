// tests/simt/emu_early_top.cpp -- TEST INFRASTRUCTURE: k_gram_downdate of csrc/dhqr_recon.h (unmodified source) on the
// CPU SIMT emulator (ThreadSanitizer build: a missing barrier between the chunks of R shows up as a data race).
// Driven by tests/test_early_top_cpu.py:
//   emu_early_top downdate <nrows> <ldr> Gold R outG        Gold, outG: 128 x 128; R: ldr x 128, column-major raw float64
//   emu_early_top downdate_stopped <nrows> <ldr> Gold R outG   the same launch with (stat, epoch) of a rejected run: a no-op
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "dhqr_recon.h"

static std::vector<double> rd(const char *path, size_t n) {
  std::vector<double> v(n);
  FILE *f = fopen(path, "rb");
  if (!f || fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fclose(f);
  return v;
}
static void wr(const char *path, const std::vector<double> &v) {
  FILE *f = fopen(path, "wb");
  if (!f || fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}

int main(int argc, char **argv) {
  if (argc < 7) return 2;
  const std::string op = argv[1];
  const int nrows = atoi(argv[2]);
  const int64_t ldr = atoll(argv[3]);
  const size_t NN = RC_N * RC_N;
  if (op != "downdate" && op != "downdate_stopped") return 2;
  auto Gold = rd(argv[4], NN);
  auto R = rd(argv[5], (size_t)ldr * RC_N);
  std::vector<double> G(NN, -7.0);
  int stat[2] = {op == "downdate" ? 1 << 30 : 3, 0};  // stopped: panel 3 was rejected, this launch carries epoch 5
  simt::launch_grid(64, 1, 256, [&] { k_gram_downdate(Gold.data(), R.data(), ldr, nrows, G.data(), stat, 5); });
  wr(argv[6], G);
  return 0;
}
