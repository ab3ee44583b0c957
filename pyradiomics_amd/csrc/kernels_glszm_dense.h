// kernels_glszm_dense.h -- GLSZM zones (cmatrices.c:94-297) in the DENSE model: the packed-byte kernels of segment mode
// (<= 3-D, the full 26- or in-plane 8-neighbourhood, levels 1..255).
//   glszm_tile8_kernel        zones labelled inside 8 x 8 x 64 tiles in LDS; every tile component gets a dense id, vid[voxel];
//                             same-level neighbours in OTHER tiles that no in-tile neighbour ties to the voxel: a work list
//   glszm_dense_init_kernel   parent[id] = id, zsize[id] = voxels of the tile component
//   glszm_pairs_kernel        union-find over the dense ids along the work list (glszm_border8d_kernel: when it overflowed)
//   glszm_rootsum_dense_kernel  counts folded into the zone roots, parent[] shortened (nearly flat: see the kernel)
// kernels_glszm_zones.h walks the ids (a zone = an id with parent[id] == id; level in tinfo[id] >> 16).  The ordered zone list
// (tempData parity, cmatrices.c:255-258) needs the first voxel of every zone: glszm_zmin_kernel, glszm_publish_kernel, on demand.
#pragma once
#include "kernels_glszm_labels.h"     // the tile, lds_find / lds_union

namespace prad {
// ---- packed-byte variants (levels 1..255 as uint8, 0 = outside the ROI; the volume pack_levels writes for the
// GLDM / NGTDM kernels) for the full 26- (MODE 1) / in-plane 8-neighbourhood (MODE 2).
// Tile kernel: a lane owns 4 x-adjacent voxels (one LDS dword).  The tile sits in LDS with a halo (one plane above, one row
// either side in y, one dword either side in x), so no bounds are tested.  For each of the 4 (dz, dy) rows of backward
// neighbours the lane reads 3 dwords and derives the "same level" flags of its 4 voxels with packed-byte arithmetic -- ~27
// VALU and ~4 LDS reads per voxel instead of 13 neighbours x (bounds test, address, two LDS reads, compare).
#define PRAD_T8_ROWDW (PRAD_TX / 4 + 2)                       // dwords per padded LDS row
#define PRAD_T8_DW ((PRAD_TZ + 1) * (PRAD_TY + 2) * PRAD_T8_ROWDW)
// The 13 backward neighbours of a voxel as bit positions n:  n = 3r + (dx + 1) for the backward rows
//   r = 0: (dz 0, dy -1)   1: (dz -1, dy -1)   2: (dz -1, dy 0)   3: (dz -1, dy +1),   and n = 12: (0, 0, -1).
__device__ __forceinline__ void t8_offset(int n, int &dz, int &dy, int &dx) {
  const int r = (n * 11) >> 5;                       // n / 3 for n < 16
  dz = (n >= 3 && n < 12) ? -1 : 0;
  dy = n >= 12 ? 0 : (r == 0 ? -1 : r - 2);
  dx = n >= 12 ? -1 : n - 3 * r - 1;
}
// One neighbour per 26-adjacency CLUSTER of the same-level backward neighbours (scripts/gen_glszm_sel13.py has the
// argument): on structured volumes nearly all 13 neighbours of a voxel have its level and form one cluster -- one union
// instead of the two (own plane, plane above) the redundancy rules of glszm_tile_kernel ask for, and none at all for a
// voxel whose left neighbour in its own quad has its level (bit 12 represents its cluster; the tile kernel ties the two
// through the initial label).
__device__ const unsigned short t8_sel13[1 << 13] = {
#include "glszm_sel13.inc"
};

// The neighbours (13 bits, numbering above) that are members of T or 26-adjacent to a member of T: rows r0..r2 see each
// other and r2 sees r3 at |dx| <= 1, the voxel to the left (bit 12) sees dx = -1 and 0 of every row.  Two sets at once
// (13-bit fields at bits 0 and 16 of T).
__device__ __forceinline__ unsigned t8_closed_nbhd2(unsigned T) {
  const unsigned W = T & 0x0fff0fffu;
  const unsigned U = W | ((W << 1) & 0x0db60db6u) | ((W >> 1) & 0x06db06dbu);
  const unsigned a = (U | (U >> 3) | (U >> 6)) & 0x00070007u, g3 = (U >> 9) & 0x00070007u, g2 = (U >> 6) & 0x00070007u;
  unsigned N = a | (a << 3) | ((a | g3) << 6) | ((g2 | g3) << 9);
  N |= ((T >> 12) & 0x00010001u) * 0x16dbu;                                   // the voxel to the left sees dx = -1, 0 of every row
  N |= (((W & 0x06db06dbu) + 0x7fff7fffu) & 0x80008000u) >> 3;                // ... and they see it
  return N;
}

#define PRAD_T8_JUMPS 3
#define PRAD_T8_FLOOD 2
#define PRAD_GZ_TILE_ROOTS 1024    // roots per tile the tile-root list takes (glszm_tile8_kernel)
// ---- the dense model of the packed-byte path ------------------------------------------------------------------------
// The tile is loaded WITH its halo of real levels, so a voxel sees the same-level backward neighbours S it has in the
// whole volume.  Those inside the tile (IN) are united here, in LDS.  A neighbour in another tile only matters when its
// 26-adjacency cluster of S has no member inside the tile: the members of a cluster are tied to each other by their own
// (earlier) unions, and the voxel reaches a cluster with a member in the tile through that member.  Clusters of S made of
// other-tile voxels only are components of Y = (S outside the tile) minus everything adjacent to IN; one representative
// of every component of Y goes to the work list (a component of Y that belongs to a cluster reached otherwise costs a
// redundant union, never a wrong one).
//
// Every tile-local component (a "tile root") gets a DENSE id -- its position in the list of tile roots:
//     vid[voxel]   = dense id of the voxel's tile root, -1 outside the ROI      (int32 [n], the only per-voxel output)
//     tinfo[id]    = voxels of the tile component (<= 4096) | grey level << 16   (ONE store per root)
//     worklist     = pairs (dense id of a voxel's tile root, linear index of a same-level neighbour in another tile)
// and glszm_dense_init_kernel, a stream over the ids, sets parent[id] = id and zsize[id] = the component's voxels
// so that what follows -- uniting tile roots across tile faces (glszm_pairs_kernel), folding the counts into the zone
// roots, zone statistics, the fill -- chases pointers in arrays of ~7 M entries (512^3 smooth: 30 MB, cache resident)
// instead of the 537 MB label volume: 18 M pairs x ~7 dependent 4-byte reads were 1.4 - 1.7 ms of random sectors there.
// rootctl[0] = tile roots, rootctl[2] = pairs written, rootctl[3] != 0: the work list was too small and
// glszm_border8d_kernel scans the tile faces instead.
template <int MODE>
__global__ void __launch_bounds__(256) glszm_tile8_kernel(const uint8_t *__restrict__ L, int Nz, int Ny, int Nx,
                                                          int *__restrict__ vid, const int *__restrict__ flags,
                                                          int *__restrict__ rootctl, unsigned *__restrict__ tinfo,
                                                          int2 *__restrict__ worklist, int workcap) {
  __shared__ unsigned lev[PRAD_T8_DW];
  __shared__ int lab[PRAD_TVOX];
  __shared__ int lcount, lbase, wcount, wbase;
  __shared__ int offt[16];                   // in-tile index offset of neighbour n (t8_offset)
  if (flags[0]) return;   // a masked level outside 1..Ng: the int32 kernels redo this call
  if (threadIdx.x < 16) {
    int dz, dy, dx;
    t8_offset(threadIdx.x, dz, dy, dx);
    offt[threadIdx.x] = threadIdx.x < 13 ? dz * (PRAD_TX * PRAD_TY) + dy * PRAD_TX + dx : 0;
  }
  const int tx = (Nx + PRAD_TX - 1) / PRAD_TX, ty = (Ny + PRAD_TY - 1) / PRAD_TY;
  const int bz = blockIdx.x / (ty * tx), br = blockIdx.x % (ty * tx);
  const int z0 = bz * PRAD_TZ, y0 = (br / tx) * PRAD_TY, x0 = (br % tx) * PRAD_TX;
  const bool vec = (Nx & 3) == 0;   // every quad is a 4-byte aligned dword of the volume (and of the vid rows)
  if (threadIdx.x == 0) lcount = wcount = 0;
  for (int i = threadIdx.x; i < PRAD_T8_DW; i += blockDim.x) {
    const int c = i % PRAD_T8_ROWDW, rw = (i / PRAD_T8_ROWDW) % (PRAD_TY + 2), pl = i / (PRAD_T8_ROWDW * (PRAD_TY + 2));
    const int z = z0 + pl - 1, y = y0 + rw - 1, x = x0 + 4 * (c - 1);
    unsigned w = 0u;
    if ((MODE == 1 || pl > 0) && (unsigned)z < (unsigned)Nz && (unsigned)y < (unsigned)Ny && x >= 0 && x < Nx) {
      const long long gi = ((long long)z * Ny + y) * Nx + x;
      if (vec) w = *reinterpret_cast<const unsigned *>(L + gi);
      else
        for (int b = 0; b < 4; b++)
          if (x + b < Nx) w |= (unsigned)L[gi + b] << (8 * b);
    }
    lev[i] = w;
  }
  __syncthreads();
  constexpr int QPT = PRAD_TVOX / 4 / 256;   // quads per lane
  unsigned cw[QPT];
  unsigned long long btodo[QPT];             // bit 16k + n of [q]: voxel k of quad q goes to the work list with its neighbour n
#pragma unroll
  for (int q = 0; q < QPT; q++) {
    const int quad = threadIdx.x + q * 256;
    const int lx4 = quad & 15, ly = (quad >> 4) % PRAD_TY, lz = quad / (16 * PRAD_TY);
    const unsigned w = lev[((lz + 1) * (PRAD_TY + 2) + (ly + 1)) * PRAD_T8_ROWDW + 1 + lx4];
    cw[q] = w;
  }
  // ---- selection.  Every voxel takes ONE of the neighbours it has to be united with (one per 26-adjacency cluster of its
  // same-level backward neighbours inside the tile: t8_sel13) as its initial label -- a plain store to its own cell, links
  // only go to smaller indices -- and keeps the others (`todo`: 0.13 per voxel on smooth volumes where uniting with every
  // representative took 0.78 finds + atomics) for the union phase.
  unsigned long long todo[QPT];              // bit 16k + n of [q]: unite voxel k of quad q with its neighbour n
#pragma unroll
  for (int q = 0; q < QPT; q++) {
    const unsigned centre = cw[q];
    btodo[q] = 0ull;
    todo[q] = 0ull;
    const int quad0 = threadIdx.x + q * 256;
    if (!centre) {
      *reinterpret_cast<int4 *>(lab + quad0 * 4) = make_int4(quad0 * 4, quad0 * 4 + 1, quad0 * 4 + 2, quad0 * 4 + 3);
      continue;
    }
    const int quad = threadIdx.x + q * 256;
    const int lx4 = quad & 15, ly = (quad >> 4) % PRAD_TY, lz = quad / (16 * PRAD_TY);
    const unsigned *row0 = lev + ((lz + 1) * (PRAD_TY + 2) + (ly + 1)) * PRAD_T8_ROWDW + lx4;   // [0] left, [1] mid, [2] right
    // "Same level" flags of the 4 voxels against one neighbour direction at a time, packed-byte arithmetic on the whole
    // dword (bit 7 of byte k: voxel k has the level of that neighbour), gathered into Wlo / Whi: byte k of Wlo = bits 0..7,
    // byte k of Whi = bits 8..12 of voxel k's set S (numbering of t8_offset).  ~30 VALU per voxel where the per-voxel
    // 3-byte windows took ~60; the kernel is bound by instruction issue (4 000 instructions per wave and tile).
    auto eq4 = [](unsigned a, unsigned b) -> unsigned {
      const unsigned x = a ^ b;
      return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    };
    unsigned Wlo = 0u, Whi = 0u;
#pragma unroll
    for (int r = 0; r < (MODE == 1 ? 4 : 1); r++) {
      const int dz = r == 0 ? 0 : -1, dy = r == 0 ? -1 : r - 2;
      const unsigned *rp = row0 + (dz * (PRAD_TY + 2) + dy) * PRAD_T8_ROWDW;
      const unsigned left = rp[0], mid = rp[1], right = rp[2];
      const unsigned em = eq4(centre, __builtin_amdgcn_alignbyte(mid, left, 3));    // dx = -1
      const unsigned e0 = eq4(centre, mid);
      const unsigned ep = eq4(centre, __builtin_amdgcn_alignbyte(right, mid, 1));   // dx = +1
#pragma unroll
      for (int d = 0; d < 3; d++) {
        const int n = 3 * r + d;
        const unsigned e = d == 0 ? em : (d == 1 ? e0 : ep);
        if (n < 8) Wlo |= e >> (7 - n);
        else Whi |= e >> (7 - (n - 8));
      }
    }
    Whi |= eq4(centre, __builtin_amdgcn_alignbyte(centre, row0[0], 3)) >> 3;        // n = 12: the voxel to the left
    {
      const unsigned nz = (((centre & 0x7f7f7f7fu) + 0x7f7f7f7fu) | centre) & 0x80808080u;
      const unsigned inroi = (nz >> 7) * 0xffu;                  // 0xff in the bytes of voxels inside the ROI
      Wlo &= inroi;
      Whi &= inroi;
    }
    // the neighbours of this row that lie in another tile
    const unsigned rowcross = (lz == 0 ? 0xff8u : 0u) | (ly == 0 ? 0x3fu : 0u) | (ly == PRAD_TY - 1 ? 0xe00u : 0u);
    unsigned IN[4], X[4];
    int ilab[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const unsigned S = __builtin_amdgcn_ubfe(Wlo, 8 * k, 8) | (__builtin_amdgcn_ubfe(Whi, 8 * k, 5) << 8);
      const unsigned cross = rowcross | ((k == 0 && lx4 == 0) ? 0x1249u : 0u) | ((k == 3 && lx4 == 15) ? 0x924u : 0u);
      X[k] = S & cross;
      IN[k] = S & ~cross;
      // (a set of at most one neighbour is its own selection: only the lanes with two or more go to the table -- a gather
      // from global memory costs the vector L1 one tag look-up per active lane)
      unsigned sel = IN[k];
      if (sel & (sel - 1u)) sel = (unsigned)t8_sel13[sel];
      // the initial label: the voxel to the left when it is one of them (runs along x become chains the jumping rounds
      // flatten), else the first in bit order
      const unsigned pick = (sel & 0x1000u) ? 0x1000u : (sel & (0u - sel));
      ilab[k] = quad * 4 + k + (pick ? offt[__ffs((int)pick) - 1] : 0);
      todo[q] |= (unsigned long long)(sel ^ pick) << (16 * k);
    }
    *reinterpret_cast<int4 *>(lab + quad * 4) = make_int4(ilab[0], ilab[1], ilab[2], ilab[3]);
    // the work list: Y = X minus everything adjacent to IN, two voxels per word (fields at bits 0 and 16)
#pragma unroll
    for (int h = 0; h < 2; h++) {
      // (PRAD_T8_FLOOD rounds of "grow through S": 1 = everything adjacent to IN, 4 = the exact clusters)
      const unsigned S2 = (IN[2 * h] | X[2 * h]) | ((IN[2 * h + 1] | X[2 * h + 1]) << 16);
      unsigned N2 = IN[2 * h] | (IN[2 * h + 1] << 16);
#pragma unroll
      for (int r = 0; r < PRAD_T8_FLOOD; r++) N2 = S2 & t8_closed_nbhd2(N2);
      const unsigned Ya = X[2 * h] & ~N2, Yb = X[2 * h + 1] & ~(N2 >> 16);
      unsigned sa = Ya, sb = Yb;
      if (sa & (sa - 1u)) sa = (unsigned)t8_sel13[sa];
      if (sb & (sb - 1u)) sb = (unsigned)t8_sel13[sb];
      btodo[q] |= ((unsigned long long)sa << (32 * h)) | ((unsigned long long)sb << (32 * h + 16));
    }
  }
  __syncthreads();
  // ---- pointer jumping: label <- label of the label, every voxel, PRAD_T8_JUMPS rounds (any interleaving of these
  // stores is valid: a label only moves to a smaller member of the same component)
#pragma unroll 1
  for (int round = 0; round < PRAD_T8_JUMPS; round++) {
#pragma unroll
    for (int q = 0; q < QPT; q++) {
      if (!cw[q]) continue;
      int4 *cell = reinterpret_cast<int4 *>(lab + (threadIdx.x + q * 256) * 4);
      const int4 p = *cell;
      volatile lds_int_t *l = (volatile lds_int_t *)lab;
      *cell = make_int4(l[p.x], l[p.y], l[p.z], l[p.w]);
    }
  }
  __syncthreads();
  // ---- the unions that are left
#pragma unroll
  for (int q = 0; q < QPT; q++) {
    const int quad = threadIdx.x + q * 256;
    unsigned long long t = todo[q];
    while (t) {
      const int bit = __ffsll((long long)t) - 1;
      t &= t - 1;
      const int idx = quad * 4 + (bit >> 4);
      lds_union(lab, idx, idx + offt[bit & 15]);
    }
  }
  __syncthreads();
  // roots of the 16 voxels of the lane, all chases in flight together
  int root[QPT][4];
  {
    volatile lds_int_t *l = (volatile lds_int_t *)lab;
#pragma unroll
    for (int q = 0; q < QPT; q++) {
      const int4 p = *reinterpret_cast<const int4 *>(lab + (threadIdx.x + q * 256) * 4);
      root[q][0] = p.x; root[q][1] = p.y; root[q][2] = p.z; root[q][3] = p.w;
    }
    bool moving = true;
    while (__any(moving)) {
      moving = false;
#pragma unroll
      for (int q = 0; q < QPT; q++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int nx = l[root[q][k]];
          moving = moving || nx != root[q][k];
          root[q][k] = nx;
        }
    }
#pragma unroll
    for (int q = 0; q < QPT; q++)
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (!((cw[q] >> (8 * k)) & 0xffu)) root[q][k] = -1;
  }
  __syncthreads();
  unsigned *cnt = reinterpret_cast<unsigned *>(lab);          // the roots are in registers: lab becomes the counts
  for (int k = threadIdx.x; k < PRAD_TVOX; k += blockDim.x) cnt[k] = 0u;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < QPT; q++) {
    int prev = -1;
    unsigned run = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int r = root[q][k];
      if (r != prev) {
        if (prev >= 0) atomicAdd(cnt + prev, run);
        prev = r;
        run = 0;
      }
      run++;
    }
    if (prev >= 0) atomicAdd(cnt + prev, run);
  }
  __syncthreads();
  // dense ids: the roots this lane owns, a block of the tile-root list for the tile, a block of the work list
  int nroots = 0, npairs = 0;
#pragma unroll
  for (int q = 0; q < QPT; q++) {
#pragma unroll
    for (int k = 0; k < 4; k++) nroots += root[q][k] == (threadIdx.x + q * 256) * 4 + k ? 1 : 0;
    npairs += __popcll(btodo[q]);
  }
  int mypos = nroots ? atomicAdd(&lcount, nroots) : 0;
  int wpos = npairs ? atomicAdd(&wcount, npairs) : 0;
  __syncthreads();
  // (one atomic per tile and list on one address each: 65 k at 512^3.  They are only harmless behind __syncthreads(), which
  // also waits for the wave's global stores -- with a barrier that orders LDS traffic alone, or with workgroups that walk
  // many tiles, the same atomics took 3.6 ms; profiles/r04_probes.md section 11)
  if (threadIdx.x == 0) {
    lbase = lcount > 0 ? atomicAdd(rootctl, lcount) : 0;       // (the arrays hold n entries: no overflow)
    wbase = -1;
    if (wcount > 0 && !__builtin_nontemporal_load(rootctl + 3)) {       // (workcap <= 2^30: the counter cannot wrap)
      const int at = atomicAdd(rootctl + 2, wcount);
      if (at < 0 || at > workcap - wcount) atomicOr(rootctl + 3, 1);     // (the list is full: glszm_border8d_kernel takes over)
      else wbase = at;
    }
  }
  __syncthreads();
  if (nroots) {
    int id = lbase + mypos;
#pragma unroll
    for (int q = 0; q < QPT; q++) {
      const int quad = threadIdx.x + q * 256;
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (root[q][k] == quad * 4 + k) {
          const unsigned sz = cnt[quad * 4 + k];             // <= 4096
          tinfo[id] = sz | (((cw[q] >> (8 * k)) & 0xffu) << 16);     // (one store per root: four cost 0.75 ms on 512^3 noise)
          lab[quad * 4 + k] = id;                              // (its count is in the dense array now)
          id++;
        }
    }
  }
  __syncthreads();
  const int plane = Ny * Nx;
#pragma unroll
  for (int q = 0; q < QPT; q++) {
    const int quad = threadIdx.x + q * 256;
    const int lx4 = quad & 15, ly = (quad >> 4) % PRAD_TY, lz = quad / (16 * PRAD_TY);
    const int z = z0 + lz, y = y0 + ly, x = x0 + 4 * lx4;
    if (z >= Nz || y >= Ny || x >= Nx) continue;
    const long long gi = ((long long)z * Ny + y) * Nx + x;
    int lb[4];
#pragma unroll
    for (int k = 0; k < 4; k++) lb[k] = root[q][k] >= 0 ? lab[root[q][k]] : -1;
    if (vec) {
      *reinterpret_cast<int4 *>(vid + gi) = make_int4(lb[0], lb[1], lb[2], lb[3]);
    } else {
      for (int k = 0; k < 4; k++)
        if (x + k < Nx) vid[gi + k] = lb[k];
    }
    unsigned long long b = btodo[q];
    if (wbase < 0) b = 0ull;
    while (b) {
      const int bit = __ffsll((long long)b) - 1;
      b &= b - 1;
      int dz, dy, dx;
      t8_offset(bit & 15, dz, dy, dx);
      worklist[wbase + wpos++] = make_int2(lb[bit >> 4], (int)gi + (bit >> 4) + dz * plane + dy * Nx + dx);
    }
  }
}

// find / union in the dense parent array (smaller id = closer to the root, as in the label volume)
__device__ __forceinline__ int dn_load(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
// (dn_union does not halve the paths it walks: with thousands of lanes in the same trees the halving stores cost more
// than the shorter chains gain -- 676 -> 612 us at 512^3 smooth; glszm_rootsum_dense_kernel flattens afterwards)
__device__ __forceinline__ int dn_find(int *parent, int i) {
  int p = dn_load(parent + i);
  while (p != i) {
    const int g = dn_load(parent + p);
    if (g != p) parent[i] = g;
    i = p;
    p = g;
  }
  return i;
}
__device__ __forceinline__ void dn_union(int *parent, int a, int b) {     // both finds in flight together
  while (true) {
    int pa = dn_load(parent + a), pb = dn_load(parent + b);
    while (pa != a || pb != b) {
      const int ga = dn_load(parent + pa), gb = dn_load(parent + pb);
      if (pa != a) { a = pa; pa = ga; }
      if (pb != b) { b = pb; pb = gb; }
    }
    if (a == b) return;
    if (a < b) { int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

// The work list: one lane per pair.  A pair of tile roots that repeats the previous lane's (neighbouring voxels of the
// same two tile components) is skipped.
__global__ void __launch_bounds__(256) glszm_pairs_kernel(const int2 *__restrict__ worklist,
                                                          const int *__restrict__ rootctl, const int *__restrict__ vid,
                                                          int *__restrict__ parent, const int *__restrict__ flags) {
  if (flags[0] || rootctl[3]) return;
  const int total = rootctl[2];
  const int stride = gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  // the pair of the NEXT round is fetched (list entry, then the neighbour's id: two dependent loads) while this round's
  // union chases its pointers: the kernel is a chain of memory latencies, 97 % of its wave cycles are waits
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int a = -1, b = -1;
  if (j < total) {
    const int2 p = worklist[j];
    a = p.x;
    b = vid[p.y];
  }
  for (int j0 = blockIdx.x * blockDim.x; j0 < total; j0 += stride) {      // (whole waves stay in the loop: shuffles)
    const int jn = j + stride;
    int an = -1, bn = -1;
    if (jn < total) {
      const int2 p = worklist[jn];
      an = p.x;
      bn = vid[p.y];
    }
    const int pa = __shfl_up(a, 1), pb = __shfl_up(b, 1);
    if (a >= 0 && a != b && !(lane > 0 && pa == a && pb == b)) dn_union(parent, a, b);
    j = jn;
    a = an;
    b = bn;
  }
}

// The route of a full work list: the faces of the tiles scanned on the level volume, one voxel per lane, the redundancy
// rules of glszm_border_full_kernel on GLOBAL sameness (a superset of what the work list would have held).
template <int MODE>
__global__ void __launch_bounds__(256) glszm_border8d_kernel(const uint8_t *__restrict__ L, int Nz, int Ny, int Nx,
                                                             const int *__restrict__ vid, int *__restrict__ parent,
                                                             const int *__restrict__ flags,
                                                             const int *__restrict__ rootctl) {
  if (flags[0] || !rootctl[3]) return;
  const int lane = threadIdx.x & 63;
  const long long nrows = (long long)Nz * Ny;
  const long long wave0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const int xtiles = (Nx + PRAD_TX - 1) / PRAD_TX;
  for (long long row = wave0; row < nrows; row += nwaves) {
    const int z = (int)(row / Ny), y = (int)(row - (long long)z * Ny);
    const bool row_edge = (MODE == 1 && z % PRAD_TZ == 0) || (y % PRAD_TY == 0) || (MODE == 1 && y % PRAD_TY == PRAD_TY - 1);
    const int count = row_edge ? Nx : 2 * xtiles;
    const long long rbase = row * Nx;
    for (int c0 = 0; c0 < count; c0 += 64) {
      const int c = c0 + lane;
      int x = -1;
      if (c < count) x = row_edge ? c : (c >> 1) * PRAD_TX + ((c & 1) ? PRAD_TX - 1 : 0);
      int gl = 0, li = -1;
      if (x >= 0 && x < Nx) {
        gl = L[rbase + x];
        if (gl) li = vid[rbase + x];
      }
      if (__ballot(li >= 0) == 0ull) continue;
      auto same = [&](int dz, int dy, int dx) -> long long {
        const int qz = z + dz, qy = y + dy, qx = x + dx;
        if ((unsigned)qz >= (unsigned)Nz || (unsigned)qy >= (unsigned)Ny || (unsigned)qx >= (unsigned)Nx) return -1;
        const long long j = ((long long)qz * Ny + qy) * Nx + qx;
        return L[j] == gl ? j : -1;
      };
      auto pair = [&](long long j, int dz, int dy, int dx) {
        int lj = -1;
        if (j >= 0) {
          const int qz = z + dz, qy = y + dy, qx = x + dx;
          const bool same_tile = qz / PRAD_TZ == z / PRAD_TZ && qy / PRAD_TY == y / PRAD_TY && qx / PRAD_TX == x / PRAD_TX;
          if (!same_tile) lj = vid[j];
        }
        const int pi = __shfl_up(li, 1), pj = __shfl_up(lj, 1);
        if (lj >= 0 && !(lane > 0 && pi == li && pj == lj)) dn_union(parent, li, lj);
      };
      const bool live = li >= 0;
      const long long jb = live ? same(0, -1, 0) : -1;
      pair(jb, 0, -1, 0);
      const bool nb = live && jb < 0;
      const long long jc = nb ? same(0, -1, 1) : -1;
      pair(jc, 0, -1, 1);
      const long long ja = nb ? same(0, -1, -1) : -1;
      pair(ja, 0, -1, -1);
      const long long jd = (nb && ja < 0) ? same(0, 0, -1) : -1;
      pair(jd, 0, 0, -1);
      if (MODE == 1) {
        const long long jm = live ? same(-1, 0, 0) : -1;
        pair(jm, -1, 0, 0);
        const bool nm = live && jm < 0;
        const long long e1 = nm ? same(-1, -1, 0) : -1, e2 = nm ? same(-1, 1, 0) : -1;
        const long long e3 = nm ? same(-1, 0, -1) : -1, e4 = nm ? same(-1, 0, 1) : -1;
        pair(e1, -1, -1, 0);
        pair(e2, -1, 1, 0);
        pair(e3, -1, 0, -1);
        pair(e4, -1, 0, 1);
        pair((nm && e1 < 0 && e3 < 0) ? same(-1, -1, -1) : -1, -1, -1, -1);
        pair((nm && e1 < 0 && e4 < 0) ? same(-1, -1, 1) : -1, -1, -1, 1);
        pair((nm && e2 < 0 && e3 < 0) ? same(-1, 1, -1) : -1, -1, 1, -1);
        pair((nm && e2 < 0 && e4 < 0) ? same(-1, 1, 1) : -1, -1, 1, 1);
      }
    }
  }
}

__global__ void __launch_bounds__(256) glszm_dense_init_kernel(const int *__restrict__ rootctl, const unsigned *__restrict__ tinfo,
                                                               int *__restrict__ parent, unsigned *__restrict__ zsize,
                                                               const int *__restrict__ flags) {
  if (flags[0]) return;
  const int m = rootctl[0], m4 = m >> 2;           // 16 B per lane and access (the streams over the ids: noise has 85 M of them)
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (int q = gid; q < m4; q += stride) {
    const uint4 ti = reinterpret_cast<const uint4 *>(tinfo)[q];
    reinterpret_cast<int4 *>(parent)[q] = make_int4(4 * q, 4 * q + 1, 4 * q + 2, 4 * q + 3);
    reinterpret_cast<uint4 *>(zsize)[q] = make_uint4(ti.x & 0xffffu, ti.y & 0xffffu, ti.z & 0xffffu, ti.w & 0xffffu);
  }
  for (int j = 4 * m4 + gid; j < m; j += stride) {
    parent[j] = j;
    zsize[j] = tinfo[j] & 0xffffu;
  }
}

// Counts of the tile components folded into their zone roots: one find per tile root in the dense array; contributions
// to the same zone root are combined in an LDS hash table first (a zone that spans thousands of tiles would otherwise
// receive thousands of atomics on one address).  parent[] is NEARLY flat afterwards: every entry was pointed at its zone
// root, but the path-halving stores of another lane's dn_find (a grandparent read before that) may land later and leave an
// entry at an ancestor short of the root -- on chains of five and more tile components.  An entry j is a zone root iff
// parent[j] == j; whoever needs the root of another entry walks the (short) rest of the chain (glszm_zmin_kernel).
#define PRAD_RS_PROBES 2      // (dense kernel; on noise the table fills up and every further probe is a wasted LDS atomic)
__global__ void __launch_bounds__(256) glszm_rootsum_dense_kernel(const int *__restrict__ rootctl, int *__restrict__ parent,
                                                                  unsigned *__restrict__ tsize,
                                                                  const int *__restrict__ flags) {
  __shared__ int hkey[PRAD_RS_SLOTS];
  __shared__ unsigned hval[PRAD_RS_SLOTS];
  if (flags[0]) return;
  const int total = rootctl[0];
  const int per = (max(1024, (total + (int)gridDim.x - 1) / (int)gridDim.x) + 3) & ~3;
  const long long lo = (long long)blockIdx.x * per, hi = min((long long)total, lo + per);
  if (lo >= hi) return;
  for (int k = threadIdx.x; k < PRAD_RS_SLOTS; k += blockDim.x) {
    hkey[k] = -1;
    hval[k] = 0u;
  }
  __syncthreads();
  auto fold = [&](int j, int p) {
    if (p == j) return;
    const int r = dn_find(parent, p);
    parent[j] = r;
    const unsigned sz = tsize[j];
    unsigned slot = ((unsigned)r * 2654435761u) >> 22;          // 10 bits
    bool done = false;
    for (int probe = 0; probe < PRAD_RS_PROBES && !done; probe++, slot = (slot + 1) & (PRAD_RS_SLOTS - 1)) {
      const int old = atomicCAS(hkey + slot, -1, r);
      if (old == -1 || old == r) {
        atomicAdd(hval + slot, sz);
        done = true;
      }
    }
    if (!done) atomicAdd(tsize + r, sz);
  };
  // (one id per lane and round: four per lane -- a 16-byte load -- made the kernel slower, 509 -> 628 us on 512^3 noise: the
  // finds and hash updates of a lane's four ids run one after the other)
  for (int j = (int)lo + threadIdx.x; j < (int)hi; j += blockDim.x) fold(j, parent[j]);
  __syncthreads();
  for (int k = threadIdx.x; k < PRAD_RS_SLOTS; k += blockDim.x)
    if (hkey[k] >= 0 && hval[k]) atomicAdd(tsize + hkey[k], hval[k]);
}

// dense model -> the label-volume view the ordered zone list needs: the first voxel of every zone (a scan of vid[])
__global__ void __launch_bounds__(256) glszm_zmin_kernel(long long n, const int *__restrict__ vid, const int *__restrict__ parent,
                                                         int *__restrict__ zmin) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += stride) {
    const int id = vid[v];
    if (id < 0) continue;
    int r = parent[id];
    for (int p = parent[r]; p != r; p = parent[r]) r = p;      // (parent[] is only nearly flat: glszm_rootsum_dense_kernel)
    if (zmin[r] > (int)v) atomicMin(zmin + r, (int)v);
  }
}
__global__ void __launch_bounds__(256) glszm_publish_kernel(const int *__restrict__ rootctl, const int *__restrict__ parent,
                                                            const unsigned *__restrict__ tsize, const int *__restrict__ zmin,
                                                            int *__restrict__ labels, unsigned *__restrict__ zsz) {
  const int m = rootctl[0];
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x)
    if (parent[j] == j) {
      const int v = zmin[j];
      labels[v] = v;
      zsz[v] = tsize[j];
    }
}

}  // namespace prad
