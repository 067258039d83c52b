// Host program of tests/test_kde_core_cpu.py: bart_amd/csrc/kde_core.hpp built by a host compiler alone, the
// exponential std::exp.
//
//   kde_core_host kde IN OUT   IN (doubles): nrows ld nsel ngrid hasmask rule factor, cols[nsel], grid[nsel][ngrid],
//                              (hasmask) mask[nrows], x[nrows][ld].  OUT (64-bit words): pdf[nsel][ngrid] and
//                              stat[nsel][4] as doubles, then nonfinite[nsel]: kde::density, the loops the kernels run.
//   kde_core_host hpd IN OUT   IN (doubles): n p, pdf[n].  OUT (64-bit words): mask[n], threshold and included as
//                              doubles, nruns.
//   kde_core_host tile IN OUT  OUT: one word, kde::kKdeTileRows (IN is read and ignored).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../bart_amd/csrc/kde_core.hpp"

using namespace bartrt;

static bool read_all(const char *path, std::vector<double> &v) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / sizeof(double));
  const bool ok = std::fread(v.data(), sizeof(double), v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}

static int write_all(const char *path, const void *p, size_t words) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return 8;
  const bool ok = std::fwrite(p, 8, words, f) == words;
  return std::fclose(f) == 0 && ok ? 0 : 9;
}

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  std::vector<double> in;
  if (!read_all(argv[2], in)) return 3;
  if (mode == "kde") {
    const size_t head = 7;
    if (in.size() < head) return 4;
    const long nrows = (long)in[0], ld = (long)in[1];
    const int nsel = (int)in[2], ngrid = (int)in[3], hasmask = (int)in[4], rule = (int)in[5];
    const double factor = in[6];
    if (nrows < 1 || ld < 1 || nsel < 1 || nsel > hist::kMaxSel || ngrid < 1 || ngrid > kde::kMaxGrid) return 5;
    const size_t ng = (size_t)nsel * ngrid;
    if (in.size() != head + nsel + ng + (hasmask ? (size_t)nrows : 0) + (size_t)nrows * ld) return 6;
    const double *colsd = in.data() + head, *grid = colsd + nsel, *maskd = grid + ng, *x = maskd + (hasmask ? nrows : 0);
    std::vector<int> cols((size_t)nsel);
    for (int s = 0; s < nsel; s++) {
      cols[s] = (int)colsd[s];
      if (cols[s] < 0 || cols[s] >= ld) return 7;
    }
    std::vector<unsigned char> mask((size_t)nrows, 1);
    if (hasmask)
      for (long r = 0; r < nrows; r++) mask[r] = maskd[r] != 0.0;
    std::vector<double> pdf(ng), stat((size_t)nsel * 4);
    std::vector<uint64_t> nonfinite((size_t)nsel), out;
    kde::density(x, nrows, ld, hasmask ? mask.data() : nullptr, nsel, cols.data(), ngrid, grid, rule, factor, pdf.data(),
                 stat.data(), nonfinite.data(), [](double a) { return std::exp(a); });
    for (double v : pdf) out.push_back(quant::bits_of(v));
    for (double v : stat) out.push_back(quant::bits_of(v));
    out.insert(out.end(), nonfinite.begin(), nonfinite.end());
    return write_all(argv[3], out.data(), out.size());
  }
  if (mode == "tile") {
    const uint64_t rows = (uint64_t)kde::kKdeTileRows;
    return write_all(argv[3], &rows, 1);
  }
  if (mode == "hpd") {
    if (in.size() < 3 || in.size() != 2 + (size_t)in[0]) return 4;
    const int n = (int)in[0];
    const double p = in[1];
    if (!(p > 0.0 && p <= 1.0)) return 5;
    std::vector<unsigned char> mask((size_t)n);
    std::vector<uint64_t> out;
    double threshold, included;
    int nruns;
    kde::hpd_pdf(in.data() + 2, n, p, mask.data(), &threshold, &included, &nruns);
    for (unsigned char m : mask) out.push_back(m);
    out.push_back(quant::bits_of(threshold));
    out.push_back(quant::bits_of(included));
    out.push_back((uint64_t)nruns);
    return write_all(argv[3], out.data(), out.size());
  }
  return 2;
}
