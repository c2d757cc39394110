"""The column deal of a split block (csrc/split_deal.hpp: which tile columns of the warm-start congruence the leader and each of its H
helper workgroups compute), compiled for the host alone and tabulated for every block size the ping-pong variant takes."""
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
    for (int H = 0; H <= 7; ++H) {
      std::printf("%d %d %d", nt, H, split_helpers(nt, H));
      for (int h = 0; h <= H; ++h) std::printf(" %u", split_cols(nt, H, h));
      std::printf("\n");
    }
  // the c-th column of a set and the size of a set, as the kernel walks them
  for (unsigned m = 1; m < 64; ++m) {
    std::printf("set %u %d", m, split_col_count(m));
    for (int c = 0; c < split_col_count(m); ++c) std::printf(" %d", split_col_at(split_col_list(m), c));
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("deal")
    src = d / "deal_main.cpp"
    src.write_text(MAIN)
    exe = d / "deal_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(helpers.ROOT, "nn-sdp_amd", "csrc"), str(src), "-o", str(exe)])
    deal, sets = {}, {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        w = line.split()
        if w[0] == "set":
            sets[int(w[1])] = (int(w[2]), [int(x) for x in w[3:]])
        else:
            deal[(int(w[0]), int(w[1]))] = (int(w[2]), [int(x) for x in w[3:]])
    return deal, sets


def test_every_column_has_exactly_one_owner(table):
    deal, _ = table
    assert len(deal) == 6 * 8
    for (nt, H), (nhelp, masks) in deal.items():
        assert len(masks) == H + 1
        for c in range(nt):
            assert sum((m >> c) & 1 for m in masks) == 1, (nt, H, c)
        assert all(m >> nt == 0 for m in masks), (nt, H)
        assert masks[0] & 1, (nt, H)
        # H is clamped to nt - 1 per block: the helpers past that own nothing, the others something, and both sides of the
        # hand-over count the same number
        assert nhelp == min(H, nt - 1)
        assert [h for h in range(1, H + 1) if masks[h]] == list(range(1, nhelp + 1)), (nt, H)


def test_one_helper_is_the_two_workgroup_deal(table):
    deal, _ = table
    for nt in range(1, 7):
        nhelp, masks = deal[(nt, 1)]
        hc = nt // 3 if nt >= 6 else 1
        helper = sum(1 << c for c in range(1, hc + 1) if c < nt)
        assert masks[1] == helper, nt
        assert masks[0] == ((1 << nt) - 1) & ~helper, nt
        assert deal[(nt, 0)] == (0, [(1 << nt) - 1])


def test_several_helpers_leave_the_leader_column_zero_and_balance_the_chains(table):
    """column c costs nt chains of T and nt - c of B: no helper carries more than the dearest column plus the mean"""
    deal, _ = table
    for (nt, H), (nhelp, masks) in deal.items():
        if nhelp < 2:
            continue
        assert masks[0] == 1, (nt, H)
        cost = [sum(2 * nt - c for c in range(nt) if (m >> c) & 1) for m in masks[1:nhelp + 1]]
        total = sum(2 * nt - c for c in range(1, nt))
        assert max(cost) <= (2 * nt - 1) + total / nhelp, (nt, H, cost)


def test_column_sets_are_walked_in_ascending_order(table):
    _, sets = table
    for m, (count, cols) in sets.items():
        assert cols == [c for c in range(6) if (m >> c) & 1] and count == len(cols)

