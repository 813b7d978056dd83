"""The carver of the mesh processing's `work` buffers (ezrt_amd/csrc/hip/ezrt_work_carver.h) alone, under the sanitizers.

The header needs no HIP include: g++ compiles it with -fsanitize=address,undefined into a stand-alone program that reads a layout --
a list of (type, count) pieces -- carves it over a null pointer for bytes(), allocates exactly that many bytes, carves it again over
the allocation, writes the first and last element of every piece and prints each piece's offset.  The layouts are three of
ezrt_mesh.hip's, as the comments above its entry points give them (weld, boundary loops, decimation), at n = 1, 683 and 2049; the
offsets expected are summed up here.  A write past the allocation, a misaligned one or an overflow ends the program with a report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ezrt_work_carver.h"
template <class T>
static void piece(ezi::WorkCarver& w, unsigned long long count, bool real) {
  const unsigned long long at = w.offset();
  T* p = w.take<T>(count);
  if (real && count) p[0] = (T)1, p[count - 1] = (T)2;
  if (!real && p) std::abort(); // a null base carves null pieces
  if (real) printf("%llu\n", at);
}
int main() {
  std::vector<char> type;
  std::vector<unsigned long long> count;
  char t;
  unsigned long long c;
  while (scanf(" %c %llu", &t, &c) == 2) type.push_back(t), count.push_back(c);
  void* base = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    ezi::WorkCarver w(base);
    for (size_t i = 0; i < type.size(); i++) {
      if (type[i] == 'q') piece<long long>(w, count[i], pass);
      else if (type[i] == 'i') piece<int>(w, count[i], pass);
      else piece<float>(w, count[i], pass);
    }
    if (pass == 0) base = malloc(w.bytes());
    else printf("%zu\n", w.bytes());
  }
  free(base);
}
"""
SIZE = {"q": 8, "i": 4, "f": 4}


def c(x):
    return (x + 2047) // 2048


def pow2(least):
    t = 8
    while t < least:
        t *= 2
    return t


def weld(n):
    h, T = 3 * n, pow2(6 * n)
    return [("q", h + 1), ("q", h + 1), ("q", c(h) + 1), ("i", T)] + [("i", h)] * 6


def boundary(n):
    h = 3 * n
    return [("q", h + 1), ("q", h + 1), ("q", c(h) + 1), ("q", h), ("q", h), ("q", 4), ("i", h), ("i", h), ("i", h)]


def decimate(n):
    h, T, T2 = 3 * n, pow2(6 * n), pow2(2 * n)
    return [("q", h + 1), ("q", c(h) + 1), ("q", T), ("q", 3 * T), ("i", T), ("i", T), ("i", 3 * T), ("i", 3 * T), ("i", h), ("i", T2), ("i", n)]


TOTAL = {weld: lambda n: (16 * (3 * n + 1) + 8 * (c(3 * n) + 1) + 4 * pow2(6 * n) + 72 * n + 7) // 8 * 8,
         boundary: lambda n: 132 * n + 4 * (n & 1) + 8 * c(3 * n) + 56,
         decimate: lambda n: 40 * n + 8 * c(3 * n) + 64 * pow2(6 * n) + 4 * pow2(2 * n) + 16}


@pytest.fixture(scope="module")
def carver(tmp_path_factory):
    d = tmp_path_factory.mktemp("work_carver")
    src, exe = d / "work_carver.cpp", d / "work_carver"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ezrt_amd", "csrc", "hip"), "-o", str(exe), str(src)], check=True)
    return lambda pieces: subprocess.run([str(exe)], input="".join("%s %d\n" % p for p in pieces), capture_output=True, text=True)


@pytest.mark.parametrize("layout", [weld, boundary, decimate], ids=lambda f: f.__name__)
@pytest.mark.parametrize("n", [1, 683, 2049])
def test_pieces_lie_where_the_layout_puts_them(carver, layout, n):
    pieces = layout(n)
    run = carver(pieces)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    got = [int(x) for x in run.stdout.split()]
    want, at = [], 0
    for kind, count in pieces:
        want.append(at)
        at += SIZE[kind] * count
    assert got == want + [(at + 7) // 8 * 8]
    assert got[-1] == TOTAL[layout](n)                                        # the formula of the header, as tests/test_mesh_work_bytes.py


def test_a_piece_off_its_alignment_ends_the_program(carver):
    run = carver([("i", 1), ("q", 1)])
    assert run.returncode != 0 and "8-byte alignment at offset 4" in run.stderr
    assert carver([("i", 1), ("f", 3), ("q", 1)]).returncode == 0             # (the same pieces, on alignment)


def test_an_empty_layout_is_eight_byte_granular(carver):
    assert carver([]).stdout.split() == ["0"]
    assert carver([("f", 3)]).stdout.split() == ["0", "16"]
