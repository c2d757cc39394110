"""What a helper workgroup asks of the column deal in front of its load (csrc/split_deal.hpp: split_has_share, split_first_col), held
against the deal itself: for every block size the ping-pong variant takes (1 to 6 tile columns), every helper count and every helper,
the closed forms say what a walk of split_cols says.  Compiled for the host alone, as test_split_deal_cpu.py compiles the deal."""
import os
import shutil
import subprocess

import pytest

import helpers

MAIN = r"""
#include <cstdio>
#include "split_deal.hpp"
int main() {
  for (int nt = 1; nt <= 6; ++nt)
    for (int H = 0; H <= 7; ++H)
      for (int h = 0; h <= 8; ++h)
        std::printf("%d %d %d %u %d %d\n", nt, H, h, split_cols(nt, H, h), split_has_share(nt, H, h) ? 1 : 0, split_first_col(h));
  return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("first_col")
    src = d / "first_col_main.cpp"
    src.write_text(MAIN)
    exe = d / "first_col_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(helpers.ROOT, "nn-sdp_amd", "csrc"), str(src), "-o", str(exe)])
    return [tuple(int(x) for x in line.split()) for line in subprocess.check_output([str(exe)], text=True).splitlines()]


def test_a_helper_has_a_share_exactly_when_the_deal_gives_it_columns(rows):
    assert len(rows) == 6 * 8 * 9
    for nt, H, h, cols, share, _ in rows:
        assert share == (1 if h >= 1 and cols != 0 else 0), (nt, H, h)


def test_the_lowest_column_of_a_share_is_the_helper_number(rows):
    """the load of a helper starts at this column of V: below it nothing of its share reads"""
    seen = 0
    for nt, H, h, cols, share, first in rows:
        if share:
            assert first == (cols & -cols).bit_length() - 1, (nt, H, h)
            assert 1 <= first <= nt - 1, (nt, H, h)
            seen += 1
    assert seen == sum(min(H, nt - 1) for nt in range(1, 7) for H in range(8))
