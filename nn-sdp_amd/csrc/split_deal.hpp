// The column deal of a split block (ProjArgs::split), stated once: which 16-wide tile columns of T = A V and of B = V'T each of the
// 1 + H workgroups of a block computes.  Plain C++ (a test compiles it for the host alone); kernels.hip includes it for both sides.
#pragma once
#if defined(__HIPCC__)
#define NNSDP_HD __host__ __device__
#else
#define NNSDP_HD
#endif

// helpers of a block of nt tile columns that have a share when the launch runs H per block: H is clamped to nt - 1 (column 0 is the
// leader's), so a launch that holds blocks of different nt runs each with what it can use
NNSDP_HD inline int split_helpers(const int nt, const int H) { return H < nt - 1 ? (H < 0 ? 0 : H) : (nt > 1 ? nt - 1 : 0); }

// bit c set: workgroup h (0 = the leader, 1 .. H = the helpers) owns tile column c of a block of nt columns.  Every column belongs to
// exactly one workgroup, the leader always owns column 0, a helper past the clamped count owns nothing.
//   H = 1   helper: columns 1 .. hc with hc = nt / 3 from six columns on, 1 below; leader: 0 and hc + 1 .. nt - 1 (the helper gets LESS
//           than half: its hand-over - stores, count, the leader's reads - runs while the leader still computes)
//   H > 1   the leader keeps column 0 alone (nt chains of T and nt of B: one per wave, so that the Gram product of a Gram visit still
//           ends before the helpers' count arrives); column c costs nt chains of T and nt - c of B, so the columns go to the helpers
//           dearest first, back and forth (1 .. H forwards, the next H backwards, ...): nt = 6, H = 3 gives {1}, {2, 5}, {3, 4} -
//           11, 17 and 17 chains - and H = 5 one column each
NNSDP_HD inline unsigned split_cols(const int nt, const int H, const int h) {
  const unsigned all = (1u << nt) - 1u;
  const int Hc = split_helpers(nt, H);
  if (Hc == 0) return h == 0 ? all : 0u;
  if (h < 0 || h > Hc) return 0u;
  if (Hc == 1) {
    const int hc = nt >= 6 ? nt / 3 : 1;
    const unsigned helper = ((1u << hc) - 1u) << 1;
    return h == 1 ? helper : all & ~helper;
  }
  if (h == 0) return 1u;
  // (walked, not divided, and the set functions below loop-free or as short as the set: the kernel works the deal out in every wave,
  // on the scalar unit the 16 waves of a workgroup share, in front of the first chain - the first form, a division per column and
  // searches for the c-th set bit, cost a W40-D20 launch 0.8 us with one helper and 1.6 us with five)
  unsigned m = 0u;
  int who = 1, dir = 1;
  for (int c = 1; c < nt; ++c) {
    if (who == h) m |= 1u << c;
    if (dir > 0) { if (who == Hc) dir = -1; else ++who; }
    else { if (who == 1) dir = 1; else --who; }
  }
  return m;
}
// Two facts about split_cols that a helper needs in front of its load, without the walk (tests/test_split_first_col_cpu.py holds
// them against split_cols for every nt, H and h): helper h has a share exactly when h <= split_helpers(nt, H), and the lowest column
// of its share is h - the first pass of the deal goes forwards, and the one helper of H = 1 starts at column 1
NNSDP_HD inline bool split_has_share(const int nt, const int H, const int h) { return h >= 1 && h <= split_helpers(nt, H); }
NNSDP_HD inline int split_first_col(const int h) { return h; }
NNSDP_HD inline int split_col_count(const unsigned cols) { return __builtin_popcount(cols); }
// a column set (columns below 16, at most 8 of them) as a list: 4 bits per entry, ascending.  The kernel builds the list once per
// workgroup, from wave-uniform values, and then finds the column of a tile with a shift - no loop in front of a tile's chain
NNSDP_HD inline unsigned split_col_list(unsigned cols) {
  unsigned list = 0u;
  for (int i = 0; cols != 0u && i < 32; i += 4, cols &= cols - 1u) list |= (unsigned)__builtin_ctz(cols) << i;
  return list;
}
NNSDP_HD inline int split_col_at(const unsigned list, const int c) { return (int)((list >> (4 * c)) & 15u); }
