"""The wide resident CROWN bounder (max_width 128, csrc/crown_wide.hpp) as far as it can be checked without a GPU: the refusals of
nnsdp_crown_create_wide (all of them come before the GPU is touched), the validation of CrownBounder and SplitOptions, and the LDS
layout of the kernel (csrc/crown_wide_layout.hpp) enumerated by a program compiled for the host alone, as
test_split_first_col_cpu.py compiles its own: for every hidden width, every slab, row and column the offsets are distinct, stay inside
the byte count the kernel is launched with, and that count is at most the CU's 160 KB."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import crown_wide_common as wc
import helpers
import literal_common as lc
import nnsdp_amd as na
from nnsdp_amd import _lib
from nnsdp_amd import split as S

MAIN = r"""
#include <cstdio>
#include <vector>
#include "crown_wide_layout.hpp"
using namespace nnsdp;
// per (activation, hidden width W): a pass of W rows and W columns, as the identity-head pass of a W-wide layer makes it.  Prints
//   tanh W slabs rows_seen rows_twice cells collisions max_offset doubles bytes
int main() {
  for (int tanh_act = 0; tanh_act < 2; ++tanh_act) {
    const int doubles = tanh_act ? kCwDoublesTanh : kCwDoubles;
    const size_t bytes = tanh_act ? kCwLdsBytesTanh : kCwLdsBytes;
    for (int W = 1; W <= kCwCols; ++W) {
      std::vector<int> row_seen(W, 0);
      long cells = 0, collisions = 0, max_off = -1;
      int twice = 0, seen = 0;
      for (int s = 0; s < cw_slabs(W); ++s) {
        std::vector<int> used((size_t)doubles + 4096, 0);      // (room behind the end: an offset past it is counted, not written past)
        auto touch = [&](long off) {
          ++cells;
          if (off > max_off) max_off = off;
          if (off < 0 || off >= (long)used.size()) { ++collisions; return; }
          if (used[(size_t)off]++) ++collisions;
        };
        const int nr = cw_slab_rows(W, s);
        if (nr < 1 || nr > kCwRows) ++collisions;
        for (int i = 0; i < nr; ++i) {
          const int g = kCwRows * s + i;
          if (g < 0 || g >= W) { ++collisions; continue; }
          if (row_seen[g]++) ++twice;
        }
        for (int m = 0; m < 2; ++m)
          for (int t = 0; t < W; ++t)
            for (int i = 0; i < nr; ++i) touch(cw_mat_off(m, t, i));
        for (int t = 0; t < W; ++t) { touch(kCwOffDu + t); touch(kCwOffDl + t); touch(kCwOffBu + t); touch(kCwOffBj + t); if (tanh_act) touch(kCwOffBl + t); }
        for (int t = 0; t < kCwRows; ++t) { touch(kCwOffC + t); touch(kCwOffR + t); touch(kCwOffRes + t); touch(kCwOffRes + kCwRows + t); }
      }
      for (int g = 0; g < W; ++g) seen += row_seen[g] ? 1 : 0;
      std::printf("%d %d %d %d %d %ld %ld %ld %d %zu\n", tanh_act, W, cw_slabs(W), seen, twice, cells, collisions, max_off, doubles, bytes);
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def layout_rows(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("crown_wide_layout")
    src = d / "crown_wide_layout_main.cpp"
    src.write_text(MAIN)
    exe = d / "crown_wide_layout_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(helpers.ROOT, "nn-sdp_amd", "csrc"), str(src), "-o", str(exe)])
    return [tuple(int(x) for x in line.split()) for line in subprocess.check_output([str(exe)], text=True).splitlines()]


def test_layout_offsets_are_distinct_and_inside_the_launched_bytes(layout_rows):
    assert len(layout_rows) == 2 * 128
    for tanh_act, W, slabs, seen, twice, cells, collisions, max_off, doubles, nbytes in layout_rows:
        assert slabs == (W + 63) // 64, (tanh_act, W)
        assert seen == W and twice == 0, (tanh_act, W)                 # every row of the pass belongs to exactly one slab
        assert collisions == 0, (tanh_act, W)
        assert 0 <= max_off < doubles and 8 * doubles == nbytes, (tanh_act, W)
        nvec = 5 if tanh_act else 4
        assert cells == 2 * W * W + slabs * (nvec * W + 4 * 64), (tanh_act, W)
        assert nbytes <= 160 * 1024


def test_layout_byte_counts_are_the_documented_ones(layout_rows):
    assert {(r[0], r[9]) for r in layout_rows} == {(0, 137216), (1, 138240)}
    assert (2 * 64 * 128 + 4 * 128 + 4 * 64) * 8 == 137216 and 137216 + 128 * 8 == 138240


def _create_wide(xdims, max_width, nlit=0, normals=None):
    lib = _lib.load()
    net = lc.random_net(xdims, 1)
    xd = np.array(xdims, dtype=np.int32)
    Mp = np.concatenate([np.asfortranarray(Mk, dtype=np.float64).ravel(order="F") for Mk in net.Ms])
    h = C.c_void_p()
    rc = lib.nnsdp_crown_create_wide(len(xdims) - 1, xd.ctypes.data_as(_lib.c_int32_p), Mp.ctypes.data_as(_lib.c_double_p), 0, nlit,
                                     None if normals is None else normals.ctypes.data_as(_lib.c_double_p), max_width, C.byref(h))
    msg = lib.nnsdp_last_error().decode() if rc != 0 else ""
    if rc == 0:
        lib.nnsdp_crown_destroy(h)
    return rc, msg


def test_create_wide_refuses_a_hidden_width_above_128():
    rc, msg = _create_wide([2, 129, 2], 128)
    assert rc == -1 and "129" in msg and "128" in msg


def test_create_wide_refuses_an_input_or_output_above_64():
    rc, msg = _create_wide([65, 100, 2], 128)
    assert rc == -1 and "65" in msg and "64" in msg and "input" in msg
    rc, msg = _create_wide([2, 100, 65], 128)
    assert rc == -1 and "65" in msg and "64" in msg and "output" in msg


def test_create_wide_refuses_a_max_width_that_is_neither_64_nor_128():
    for mw in (96, 0, 65, 256):
        rc, msg = _create_wide([2, 10, 2], mw)
        assert rc == -1 and "max_width" in msg and str(mw) in msg


def test_create_wide_with_64_gives_the_narrow_entrys_message():
    lib = _lib.load()
    rc, msg = _create_wide([2, 65, 2], 64)
    assert rc == -1
    net = lc.random_net([2, 65, 2], 1)
    xd = np.array([2, 65, 2], dtype=np.int32)
    Mp = np.concatenate([np.asfortranarray(Mk, dtype=np.float64).ravel(order="F") for Mk in net.Ms])
    h = C.c_void_p()
    assert lib.nnsdp_crown_create(2, xd.ctypes.data_as(_lib.c_int32_p), Mp.ctypes.data_as(_lib.c_double_p), 0, 0, None, C.byref(h)) == -1
    assert msg == lib.nnsdp_last_error().decode()
    assert "65" in msg and "64" in msg


def test_create_wide_keeps_the_existing_refusals():
    rc, msg = _create_wide([2, 100, 2], 128, nlit=65, normals=np.zeros((65, 2)))
    assert rc == -1 and "nlit" in msg
    rc, msg = _create_wide([2, 100, 2], 128, nlit=1, normals=np.array([[np.nan, 0.0]]))
    assert rc == -1 and "literal 0" in msg
    rc, msg = _create_wide([2, 0, 2], 128)
    assert rc == -1 and ">= 1" in msg


def test_crown_bounder_validates_max_width_before_the_library():
    net = lc.random_net([2, 100, 2], 1)
    with pytest.raises(ValueError, match="max_width"):
        na.CrownBounder(net, None, max_width=96)
    with pytest.raises(_lib.NnsdpError, match="129"):
        na.CrownBounder(lc.random_net([2, 129, 2], 1), None, max_width=128)
    with pytest.raises(_lib.NnsdpError, match="above 64"):
        na.CrownBounder(net, None)


def test_split_options_validate_crown_max_width():
    net = lc.random_net([2, 100, 2], 1)
    lo, hi = -np.ones(2), np.ones(2)
    lits = [(np.array([1.0, -1.0]), 0.0)]
    opts = na.AdmmSdpOptions()
    assert S.SplitOptions().crown_max_width == 64
    cases = [
        (dict(crown_max_width=96, crown_backend="resident"), "64 or 128"),
        (dict(crown_max_width=128, crown_backend="host"), "resident"),
        (dict(crown_max_width=128, crown_backend="gpu"), "resident"),
        (dict(crown_max_width=128, crown_backend="resident", alpha_steps=2, literal_bounds=True), "alpha_steps"),
    ]
    for kw, pat in cases:
        with pytest.raises(ValueError, match=pat):
            S.verifySplit(net, lo, hi, lits, 0, opts, S.SplitOptions(sdp_per_level=0, **kw))
        with pytest.raises(ValueError, match=pat):
            S.reachSplit(net, lo, hi, np.array([[1.0, -1.0]]), 0.1, split=S.SplitOptions(sdp_per_level=0, **kw))


def test_the_float32_figure_of_the_host_routine_on_the_wide_nets():
    """max |R(float64) - host| / (1 + |v|) on the wide ReLU nets, without the kernel: the yardstick of the GPU test's agreement with the
    host routine (DESIGN.md section 5 records it beside the 3.1e-7 of the narrow nets)"""
    for name in wc.WIDE:      # the nets of the figure are nets the wide entry takes: past its width checks it asks for the GPU, or succeeds
        rc, msg = _create_wide(wc.SHAPES[name], 128)
        assert rc == 0 or "no HIP device" in msg, (name, msg)
    figure = wc.host_figure()
    print(f"max |R(float64) - host| / (1 + |v|) on the wide nets = {figure:.3e} (recorded {wc.HOST_FLOAT32_FIGURE_WIDE:.3e})")
    assert 0.0 < figure < 1e-4, "the host routine is float32: the figure is of float32 size"
    assert abs(figure - wc.HOST_FLOAT32_FIGURE_WIDE) <= 0.25 * wc.HOST_FLOAT32_FIGURE_WIDE, "the recorded figure is out of date"
