// Host program of tests/test_quant_core_cpu.py: bart_amd/csrc/quant_core.hpp built by a host compiler alone.
//
//   quant_core_host keys IN OUT     IN: n doubles.  OUT (64-bit words): key_of each, then bits_of_key of each key.
//   quant_core_host select IN OUT   IN (doubles): nrows ncols nranks hasmask, ranks[nranks], (hasmask) mask[nrows],
//                                   x[nrows][ncols].  OUT: out[nranks][ncols], quant::select of every column: the
//                                   repeated histogram walk the kernels run.
//   quant_core_host rule IN OUT     IN (doubles): pairs n, q.  OUT (doubles): lo, hi, w of every pair.
//   quant_core_host lerp IN OUT     IN (doubles): m, then m triples a, b, w.  OUT: quant::interpolate of every triple.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../bart_amd/csrc/quant_core.hpp"

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
  if (mode == "keys") {
    std::vector<uint64_t> out;
    for (double x : in) out.push_back(quant::key_of(x));
    for (size_t i = 0; i < in.size(); i++) out.push_back(quant::bits_of_key(out[i]));
    return write_all(argv[3], out.data(), out.size());
  }
  if (mode == "select") {
    if (in.size() < 4) return 4;
    const long nrows = (long)in[0];
    const int ncols = (int)in[1], nranks = (int)in[2], hasmask = (int)in[3];
    if (nrows < 1 || ncols < 1 || nranks < 1 || nranks > quant::kMaxRanks) return 5;
    const size_t want = 4 + (size_t)nranks + (hasmask ? (size_t)nrows : 0) + (size_t)nrows * ncols;
    if (in.size() != want) return 6;
    const double *ranks = in.data() + 4, *maskd = ranks + nranks, *x = maskd + (hasmask ? nrows : 0);
    std::vector<unsigned char> mask((size_t)nrows, 1);
    if (hasmask)
      for (long r = 0; r < nrows; r++) mask[r] = maskd[r] != 0.0;
    std::vector<double> out((size_t)nranks * ncols);
    for (int r = 0; r < nranks; r++)
      for (int c = 0; c < ncols; c++)
        out[(size_t)r * ncols + c] = quant::select(x + c, (size_t)ncols, nrows, hasmask ? mask.data() : nullptr, (long)ranks[r]);
    return write_all(argv[3], out.data(), out.size());
  }
  if (mode == "rule") {
    std::vector<double> out;
    for (size_t i = 0; i + 1 < in.size(); i += 2) {
      long lo, hi;
      double w;
      quant::percentile_rule((long)in[i], in[i + 1], &lo, &hi, &w);
      out.push_back((double)lo);
      out.push_back((double)hi);
      out.push_back(w);
    }
    return write_all(argv[3], out.data(), out.size());
  }
  if (mode == "lerp") {
    if (in.empty() || in.size() != 1 + 3 * (size_t)in[0]) return 4;
    std::vector<double> out;
    for (size_t i = 1; i < in.size(); i += 3) out.push_back(quant::interpolate(in[i], in[i + 1], in[i + 2]));
    return write_all(argv[3], out.data(), out.size());
  }
  return 2;
}
