// Host program of tests/test_hist_core_cpu.py: bart_amd/csrc/hist_core.hpp built by a host compiler alone.
//
//   hist_core_host bin IN OUT     IN (doubles): nrows ld nsel nbins hasmask wantpairs, cols[nsel], edges[nsel][nbins + 1],
//                                 (hasmask) mask[nrows], x[nrows][ld].  OUT (64-bit words): h1[nsel][nbins],
//                                 out[nsel][3], (wantpairs) h2[npairs][nbins][nbins]: hist::marginals, the loop the
//                                 kernels run.
//   hist_core_host range IN OUT   IN (doubles): nrows ld nsel hasmask, cols[nsel], (hasmask) mask[nrows], x[nrows][ld].
//                                 OUT (64-bit words): lohi[nsel][2] as doubles, then nfinite[nsel].
//   hist_core_host hpd IN OUT     IN (doubles): nbins p, counts[nbins].  OUT (64-bit words): mask[nbins], threshold,
//                                 included, nruns.
//   hist_core_host edges IN OUT   IN (doubles): nbins, e[nbins + 1].  OUT: one word, hist::bad_edge as a signed integer.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../bart_amd/csrc/hist_core.hpp"

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
  if (mode == "bin" || mode == "range") {
    const bool bin = mode == "bin";
    const size_t head = bin ? 6 : 4;
    if (in.size() < head) return 4;
    const long nrows = (long)in[0], ld = (long)in[1];
    const int nsel = (int)in[2], nbins = bin ? (int)in[3] : 0, hasmask = (int)in[bin ? 4 : 3], wantpairs = bin ? (int)in[5] : 0;
    if (nrows < 1 || ld < 1 || nsel < 1 || nsel > hist::kMaxSel || (bin && (nbins < 1 || nbins > hist::kMaxBins))) return 5;
    const size_t nedges = bin ? (size_t)nsel * (nbins + 1) : 0;
    if (in.size() != head + nsel + nedges + (hasmask ? (size_t)nrows : 0) + (size_t)nrows * ld) return 6;
    const double *colsd = in.data() + head, *edges = colsd + nsel, *maskd = edges + nedges, *x = maskd + (hasmask ? nrows : 0);
    std::vector<int> cols((size_t)nsel);
    for (int s = 0; s < nsel; s++) {
      cols[s] = (int)colsd[s];
      if (cols[s] < 0 || cols[s] >= ld) return 7;
    }
    std::vector<unsigned char> mask((size_t)nrows, 1);
    if (hasmask)
      for (long r = 0; r < nrows; r++) mask[r] = maskd[r] != 0.0;
    const unsigned char *ok = hasmask ? mask.data() : nullptr;
    if (bin) {
      const size_t n1 = (size_t)nsel * nbins, n2 = wantpairs ? (size_t)nsel * (nsel - 1) / 2 * nbins * nbins : 0;
      std::vector<uint64_t> out(n1 + (size_t)nsel * 3 + n2);
      hist::marginals(x, nrows, ld, ok, nsel, cols.data(), nbins, edges, out.data(), out.data() + n1,
                      wantpairs ? out.data() + n1 + (size_t)nsel * 3 : nullptr);
      return write_all(argv[3], out.data(), out.size());
    }
    std::vector<double> lohi((size_t)nsel * 2);
    std::vector<uint64_t> nfinite((size_t)nsel), out;
    hist::marginals_range(x, nrows, ld, ok, nsel, cols.data(), lohi.data(), nfinite.data());
    for (double v : lohi) out.push_back(quant::bits_of(v));
    out.insert(out.end(), nfinite.begin(), nfinite.end());
    return write_all(argv[3], out.data(), out.size());
  }
  if (mode == "hpd") {
    if (in.size() < 3 || in.size() != 2 + (size_t)in[0]) return 4;
    const int nbins = (int)in[0];
    const double p = in[1];
    if (!(p > 0.0 && p <= 1.0)) return 5;
    std::vector<uint64_t> counts((size_t)nbins), out;
    for (int i = 0; i < nbins; i++) counts[i] = (uint64_t)in[2 + i];
    std::vector<unsigned char> mask((size_t)nbins);
    uint64_t threshold, included;
    int nruns;
    hist::hpd(counts.data(), nbins, p, mask.data(), &threshold, &included, &nruns);
    for (unsigned char m : mask) out.push_back(m);
    out.push_back(threshold);
    out.push_back(included);
    out.push_back((uint64_t)nruns);
    return write_all(argv[3], out.data(), out.size());
  }
  if (mode == "edges") {
    if (in.size() < 3 || in.size() != 2 + (size_t)in[0]) return 4;
    const int64_t bad = hist::bad_edge(in.data() + 1, (int)in[0]);
    return write_all(argv[3], &bad, 1);
  }
  return 2;
}
