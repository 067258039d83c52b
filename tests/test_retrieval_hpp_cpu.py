"""CPU: bart_amd/csrc/retrieval.hpp alone through a host compiler: the header needs no HIP and neither core, and
check_stepsize / copy_shared read MC3's `stepsize` convention as both cores rely on it."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))

PROGRAM = r"""
#include <cstdio>
#include "%s"
int main() {
  const double shared_target[4] = {1, 0, -1, -3}, out_of_range[4] = {1, -5, 0, 0}, valid[4] = {1, 0, -1, -1};
  int nfree = -1;
  std::printf("%%d ", bartrt::check_stepsize(4, shared_target, nullptr));
  std::printf("%%d ", bartrt::check_stepsize(4, out_of_range, nullptr));
  const int refused = bartrt::check_stepsize(4, valid, &nfree);
  std::printf("%%d %%d ", refused, nfree);
  double p[4] = {2.5, 7.0, -1.0, -2.0};
  bartrt::copy_shared(4, valid, p);
  const bartrt::Objective o{4, 0, nfree, p, p, valid, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::printf("%%g %%g %%g %%g %%d\n", p[0], p[1], p[2], p[3], o.npars - o.nfree);
}
"""


def test_header_alone_reads_the_stepsize_convention(tmp_path):
    src, exe = str(tmp_path / "retrieval_host.cpp"), str(tmp_path / "retrieval_host")
    with open(src, "w") as f:
        f.write(PROGRAM % os.path.join(os.path.dirname(HERE), "bart_amd", "csrc", "retrieval.hpp"))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    # {1, 0, -1, -3}: the last parameter (index 3) names parameter 3 counted from 1, which is shared itself -> 1 + 3
    # {1, -5, 0, 0}: parameter 1 names a fifth parameter of four -> 1 + 1
    # {1, 0, -1, -1}: valid, one free parameter; both copies take parameter 0's value, the fixed one stays
    assert out == ["4", "2", "0", "1", "2.5", "7", "2.5", "2.5", "3"]
