// Whole-volume connected-component labelling and sphere painting for gfx950 (integer work, L2 / HBM bound).
// Reference: tools/evaluation/eval_instance_segmentation_soma_ngps.py, the two baselines the soma results are compared with:
//   DSN  :184-187  pred_mask = skimage.measure.label(pred_mask)  - connected components of a voxelwise segmentation as instances
//   NGPS :159-183  NeuroGPS soma lists (x, y, z, r) painted as spheres into a uint16 volume
// m3d_label_components has skimage.measure.label(x) semantics with default arguments: a component is a maximal connected set of
// voxels that share one NON-ZERO value (equal values connect, not merely "foreground"), value 0 gets label 0, and labels are 1..K in
// the raster order (z, y, x) of each component's first voxel - the order skimage, cc3d and scipy.ndimage.label all use.
//
// Algorithm: the union-find of cc3d.hip, generalised from "foreground" to "same value as me" and from 26 to 6 / 18 / 26 neighbours,
// followed by a device-wide scan that turns roots into consecutive ids.  Five launches:
//   1. lc_init    x runs of equal value are linked WITHOUT atomics: every voxel points at the first voxel of its run inside its wave;
//   2. lc_union   each voxel unions itself with its raster-PRECEDING neighbours of equal value (3 / 9 / 13 of them); atomicMin hangs
//                 the larger root under the smaller, so a component's root is its first voxel in raster order.  Redundant unions are
//                 pruned (rules and their proofs at the kernel);
//   3. lc_flatten every voxel finds its root and stores it; a root stores -(2 + its rank among the roots of its 1024-voxel block)
//                 instead, and the block's root count goes to sums[block];
//   4. lc_scan    exclusive scan of the block sums (one workgroup), K = their total;
//   5. lc_relabel label(v) = 1 + sums[block of root] + rank of root inside its block.  Roots in ascending index order ARE the raster
//                 order of first voxels, so this is the reference's numbering.
// Kernel boundaries give the visibility between the phases (no single-pass look-back scan, no in-launch hand-off between
// workgroups).  The result is a function of the input alone: the union order changes which intermediate links exist, never the root.
#include "m3d_common.h"

namespace {

constexpr int kT = 256;
constexpr int kScanBlock = 1024;        // voxels per block of the root scan: 4 sweeps of kT threads
constexpr int kScanThreads = 1024;      // lc_scan: one workgroup

// ---------------------------------------------------------------------------------------------------- union-find
// Within the union launch plain loads of `parent` may be stale (L1 is per CU and another XCD's L2 may hold an older line).  The scheme
// tolerates that: every write to parent[x] stores a value smaller than the one it replaces and in the same (final) component, so a
// stale parent is still an earlier voxel of the component and every walk terminates; a stale "root" is caught by the `old == a` test
// on the atomicMin, which returns the truth, and the union retries from there.  The flatten / relabel passes run in LATER launches
// than the last union, where every parent word is settled.
__device__ inline int uf_find_halve(int* parent, int x) {
  while (true) {
    const int p = parent[x];
    if (p == x) return x;
    const int gp = parent[p];
    if (gp != p) parent[x] = gp;     // path halving: parents only ever move towards the root, the unsynchronised store is benign
    x = p;
  }
}
__device__ inline void uf_union(int* parent, int a, int b) {
  while (true) {
    a = uf_find_halve(parent, a); b = uf_find_halve(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }      // a > b: hang root a under b
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;                                           // a was no root any more (stale view, or linked meanwhile): retry from its parent
  }
}

template <typename T>
__global__ __launch_bounds__(kT) void lc_init(const T* __restrict__ in, int V, int W, int* __restrict__ parent) {
  const int lane = threadIdx.x & 63;
  const int nloop = (int)(((long long)V + (long long)gridDim.x * kT - 1) / ((long long)gridDim.x * kT));   // uniform trip count (ballots)
  for (int it = 0; it < nloop; ++it) {
    const long long vv = ((long long)it * gridDim.x + blockIdx.x) * kT + threadIdx.x;   // a wave holds 64 consecutive voxels
    const bool inb = vv < V;
    const int v = inb ? (int)vv : 0;
    const T val = inb ? in[v] : (T)0;
    const bool fg = inb && val != (T)0;
    const int x = v % W;
    // the value one voxel to the left: from the neighbouring lane, or from memory for the wave's first lane
    const T lv = (T)__shfl_up((int)val, 1, 64);
    const bool left = fg && x > 0 && (lane ? lv == val : in[v - 1] == val);
    const bool start = fg && !left;
    const unsigned long long below = __ballot(start) & ((2ull << lane) - 1ull);
    // no run start at or below my lane: the run continues from the previous wave; point one voxel to the left of this wave (same row,
    // same value), whose own parent is the run's start there
    if (inb) parent[v] = !fg ? -1 : (below ? (v - lane) + (63 - __clzll((long long)below)) : (v - lane) - 1);
  }
}

// The raster-preceding neighbours of v, with c = v - W (previous row) and cc = v - W*H (previous plane):
//    6: v-1, c, cc                                   18: + c-1, c+1, cc-1, cc+1, cc-W, cc+W                   26: + cc-W-1, cc-W+1, cc+W-1, cc+W+1
// v-1 is linked by lc_init.  "same(n)" = voxel n holds v's value; every voxel named below has it, so all chains stay inside one value.
// Pruning rules (a skipped union is implied by others, by induction over raster order):
//  A (every connectivity)  v ~ n with n = c or cc directly behind v: skipped when v-1 and n-1 are both same.  v-1 ~ v and n-1 ~ n are x
//    links, and v-1 ~ n-1 is the same case one voxel to the left: it is made there, or skipped for the same reason, down to the first
//    voxel of the overlap of the two runs, which makes it.  One union per pair of overlapping runs instead of one per voxel.
//  B (18, 26)  in-plane diagonals c-1, c+1: not needed when c is same (both are x-linked to c, and v ~ c is case A).  With c different,
//    v ~ c-1 is skipped when v-1 is same: c-1 lies directly behind v-1, which is case A for v-1, and v-1 ~ v is an x link.
//  C (18, 26)  previous plane, cc same: v ~ cc (case A) suffices.  Every other voxel of the 3x3 block around cc that is a neighbour of v
//    is also an IN-PLANE neighbour of cc (edge neighbours at 18, edge and diagonal at 18 and 26: two coordinates differ at most), so
//    its own in-plane unions linked it to cc in this launch's final state.
//  D (26)  previous plane, cc different: per row of the block, a same row centre (dy != 0) stands for its two x neighbours; otherwise
//    both sides are united directly.  (18) cc different: the four edge neighbours cc-1, cc+1, cc-W, cc+W directly, no pruning.
template <typename T, int CONN>
__global__ __launch_bounds__(kT) void lc_union(const T* __restrict__ in, int V, int H, int W, int* __restrict__ parent) {
  const int sy = W, sz = W * H;
  const long long stride = (long long)gridDim.x * kT;
  for (long long vv = (long long)blockIdx.x * kT + threadIdx.x; vv < V; vv += stride) {
    const int v = (int)vv;
    const T val = in[v];
    if (val == (T)0) continue;
    auto same = [&](int n) __attribute__((always_inline)) { return in[n] == val; };
    const int x = v % W, y = (v / W) % H, z = v / sz;
    const bool xl = x > 0, xr = x + 1 < W;
    const bool lf = xl && same(v - 1);
    if (y > 0) {
      const int c = v - sy;
      if (same(c)) { if (!(lf && same(c - 1))) uf_union(parent, v, c); }                       // A
      else if (CONN >= 18) {                                                                   // B
        if (xl && !lf && same(c - 1)) uf_union(parent, v, c - 1);
        if (xr && same(c + 1)) uf_union(parent, v, c + 1);
      }
    }
    if (z > 0) {
      const int cc = v - sz;
      if (same(cc)) { if (!(lf && same(cc - 1))) uf_union(parent, v, cc); }                    // A, C
      else if (CONN == 18) {
        if (xl && same(cc - 1)) uf_union(parent, v, cc - 1);
        if (xr && same(cc + 1)) uf_union(parent, v, cc + 1);
        if (y > 0 && same(cc - sy)) uf_union(parent, v, cc - sy);
        if (y + 1 < H && same(cc + sy)) uf_union(parent, v, cc + sy);
      } else if (CONN == 26) {                                                                 // D
        for (int dy = -1; dy <= 1; ++dy) {
          const int yy = y + dy;
          if (yy < 0 || yy >= H) continue;
          const int c = cc + dy * sy;
          if (dy != 0 && same(c)) uf_union(parent, v, c);
          else {
            if (xl && same(c - 1)) uf_union(parent, v, c - 1);
            if (xr && same(c + 1)) uf_union(parent, v, c + 1);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- roots -> consecutive ids
// exclusive rank of a 1-bit flag over the workgroup; *total = the workgroup's count.  s: kT / 64 ints of LDS.
__device__ inline int block_rank(bool flag, int* s, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  __syncthreads();                                      // s may still be read from the previous call
  if (lane == 0) s[w] = __popcll(m);
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kT / 64; ++i) { const int c = s[i]; tot += c; before += i < w ? c : 0; }
  *total = tot;
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

// a walk that also stops at a root lc_flatten has already re-coded (parent <= -2) in this launch
__device__ inline int find_root(const int* parent, int x) {
  while (true) {
    const int p = parent[x];
    if (p == x || p < 0) return x;
    x = p;
  }
}

__global__ __launch_bounds__(kT) void lc_flatten(int* __restrict__ parent, int V, int* __restrict__ sums) {
  __shared__ int s[kT / 64];
  const long long base = (long long)blockIdx.x * kScanBlock;
  int run = 0;
#pragma unroll 1
  for (int it = 0; it < kScanBlock / kT; ++it) {
    const long long vv = base + it * kT + threadIdx.x;
    const int v = (int)vv;
    int root = -1;
    if (vv < V && parent[v] >= 0) root = find_root(parent, v);
    const bool is_root = root >= 0 && root == v;
    int tot;
    const int rank = run + block_rank(is_root, s, &tot);
    run += tot;
    if (root >= 0) parent[v] = is_root ? -(2 + rank) : root;     // rank < 1024
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = run;
}

// exclusive scan of n block sums in place by ONE workgroup; the total (K) goes to *num
__global__ __launch_bounds__(kScanThreads) void lc_scan(int* __restrict__ sums, int n, int32_t* __restrict__ num) {
  __shared__ int part[kScanThreads];
  const int per = (n + kScanThreads - 1) / kScanThreads;          // consecutive sums per thread
  const int i0 = threadIdx.x * per, i1 = min(n, i0 + per);
  int t = 0;
  for (int i = i0; i < i1; ++i) t += sums[i];
  part[threadIdx.x] = t;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {              // Hillis-Steele inclusive scan of the thread totals
    const int a = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += a;
    __syncthreads();
  }
  int run = part[threadIdx.x] - t;
  for (int i = i0; i < i1; ++i) { const int x = sums[i]; sums[i] = run; run += x; }
  if (threadIdx.x == kScanThreads - 1) *num = part[kScanThreads - 1];
}

__global__ __launch_bounds__(kT) void lc_relabel(const int* __restrict__ parent, const int* __restrict__ offs, int V,
                                                 int32_t* __restrict__ labels) {
  const long long stride = (long long)gridDim.x * kT;
  for (long long vv = (long long)blockIdx.x * kT + threadIdx.x; vv < V; vv += stride) {
    const int v = (int)vv;
    int p = parent[v], r = v;
    int lab = 0;
    if (p != -1) {
      if (p >= 0) { r = p; p = parent[r]; }                        // flattened: p is the root, whose word holds its coded rank
      lab = offs[r / kScanBlock] + (-p - 2) + 1;
    }
    labels[v] = lab;
  }
}

// ---------------------------------------------------------------------------------------------------- voxel counts per label
// Every workgroup owns a contiguous piece of the volume.  A thread folds 16 consecutive voxels into runs of equal labels in registers
// (label volumes are runs along x); a thread whose 16 voxels are ONE run - the inside of a component, the background - hands it to its
// wave, which merges equal labels first (up to 1024 voxels per add); every run then goes into the workgroup's LDS table (label ->
// count, open addressing), and the table is flushed once: one global atomic per distinct label per workgroup, never one per voxel
// and never one per run on a single address (the first version added runs to global memory directly: 13.7 ms on a random mask
// whose background and giant component take most runs, against 0.5 ms for the labelling itself).  A run that finds no slot within
// kCountProbes probes adds to global memory itself, so a full table costs time, not correctness.
constexpr int kCountPer = 16;
constexpr int kCountSlots = 2048;
constexpr int kCountProbes = 16;
__device__ inline void count_insert(int* lkey, unsigned int* lcnt, unsigned long long* counts, int label, unsigned int n) {
  unsigned int h = ((unsigned int)label * 2654435761u) >> 21;                  // top 11 bits: kCountSlots = 2^11
  for (int p = 0; p < kCountProbes; ++p) {
    const int k = atomicCAS(&lkey[h], -1, label);
    if (k == -1 || k == label) { atomicAdd(&lcnt[h], n); return; }
    h = (h + 1) & (kCountSlots - 1);
  }
  atomicAdd(&counts[label], (unsigned long long)n);
}
__global__ __launch_bounds__(kT) void lcount_kernel(const int32_t* __restrict__ labels, long long V, int K, long long per_block,
                                                    unsigned long long* __restrict__ counts) {
  __shared__ int lkey[kCountSlots];
  __shared__ unsigned int lcnt[kCountSlots];
  for (int i = threadIdx.x; i < kCountSlots; i += kT) { lkey[i] = -1; lcnt[i] = 0u; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long t0 = (long long)blockIdx.x * per_block;                     // per_block: 16-voxel items per workgroup, a multiple of kT
  for (long long it = 0; it < per_block; it += kT) {                          // uniform trip count (ballots)
    const long long t = t0 + it + threadIdx.x;
    const long long i0 = min(V, t * kCountPer), i1 = min(V, i0 + kCountPer);
    int cur = -1;
    unsigned int run = 0;
    bool mixed = false;
    for (long long i = i0; i < i1; ++i) {
      const int l = labels[i];
      if (l != cur) {
        if (run && (unsigned)cur <= (unsigned)K) count_insert(lkey, lcnt, counts, cur, run);
        mixed = mixed || run != 0;
        cur = l; run = 0;
      }
      ++run;
    }
    const bool ok = run != 0 && (unsigned)cur <= (unsigned)K;                  // a label outside [0, K] is never used as an index
    if (mixed && ok) count_insert(lkey, lcnt, counts, cur, run);
    unsigned long long todo = __ballot(ok && !mixed);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int ll = __shfl(cur, leader, 64);
      const unsigned long long samem = __ballot(ok && !mixed && cur == ll) & todo;
      unsigned int mine = ((samem >> lane) & 1ull) ? run : 0u;                 // the lanes of one label: sum their run lengths
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
      if (lane == leader) count_insert(lkey, lcnt, counts, ll, mine);
      todo &= ~samem;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kCountSlots; i += kT)
    if (lkey[i] >= 0 && lcnt[i]) atomicAdd(&counts[lkey[i]], (unsigned long long)lcnt[i]);
}

// ---------------------------------------------------------------------------------------------------- sphere painting
// eval_instance_segmentation_soma_ngps.py:165-183: sphere i (0-based) paints id i + 1 over ix in [max(1, x - r), min(W, x + r + 1)),
// likewise y / H and z / S, where (ix-x)^2 + (iy-y)^2 + (iz-z)^2 <= r^2, and only when r >= 6.  The lower clamp is 1: index 0 of every
// axis is never painted.  A later sphere overwrites an earlier one <=> every voxel keeps the HIGHEST id that covers it: atomicMax on a
// 32-bit scratch volume (independent of launch order), then narrowed to uint16.
__global__ __launch_bounds__(kT) void sphere_paint(const int32_t* __restrict__ sph, int S, int H, int W, unsigned int* __restrict__ vol32) {
  const int i = blockIdx.y;
  const long long x = sph[4 * i], y = sph[4 * i + 1], z = sph[4 * i + 2], r = sph[4 * i + 3];
  if (r < 6) return;
  const long long x0 = max(1ll, x - r), x1 = min((long long)W, x + r + 1);
  const long long y0 = max(1ll, y - r), y1 = min((long long)H, y + r + 1);
  const long long z0 = max(1ll, z - r), z1 = min((long long)S, z + r + 1);
  if (x0 >= x1 || y0 >= y1 || z0 >= z1) return;
  const long long ex = x1 - x0, ey = y1 - y0, n = ex * ey * (z1 - z0);                 // box inside the volume: n <= V < 2^31
  const unsigned long long r2 = (unsigned long long)r * (unsigned long long)r;
  for (long long t = (long long)blockIdx.x * kT + threadIdx.x; t < n; t += (long long)gridDim.x * kT) {
    const long long ix = x0 + t % ex, iy = y0 + (t / ex) % ey, iz = z0 + t / (ex * ey);
    // the box lies inside [c - r, c + r] on every axis: |d| <= r < 2^31, so the three squares sum below 2^64
    const unsigned long long dx = (unsigned long long)llabs(ix - x), dy = (unsigned long long)llabs(iy - y), dz = (unsigned long long)llabs(iz - z);
    if (dx * dx + dy * dy + dz * dz <= r2) atomicMax(&vol32[((size_t)iz * H + iy) * W + ix], (unsigned int)(i + 1));
  }
}
__global__ __launch_bounds__(kT) void sphere_narrow(const unsigned int* __restrict__ vol32, long long V, uint16_t* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < V; i += (long long)gridDim.x * kT) out[i] = (uint16_t)vol32[i];
}

int grid_for(long long items, int cap) {
  const long long b = (items + kT - 1) / kT;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <typename T>
void launch_label(const void* d_in, int V, int H, int W, int conn, int* parent, hipStream_t st) {
  const T* in = (const T*)d_in;
  const int g = grid_for(V, 8192);
  hipLaunchKernelGGL((lc_init<T>), dim3(g), dim3(kT), 0, st, in, V, W, parent);
  if (conn == 6) hipLaunchKernelGGL((lc_union<T, 6>), dim3(g), dim3(kT), 0, st, in, V, H, W, parent);
  else if (conn == 18) hipLaunchKernelGGL((lc_union<T, 18>), dim3(g), dim3(kT), 0, st, in, V, H, W, parent);
  else hipLaunchKernelGGL((lc_union<T, 26>), dim3(g), dim3(kT), 0, st, in, V, H, W, parent);
}

}  // namespace

static inline size_t label_blocks(int64_t V) { return (size_t)((V + kScanBlock - 1) / kScanBlock); }

M3D_API size_t m3d_label_components_workspace_bytes(int64_t num_voxels) {
  if (num_voxels <= 0) return 256;
  return 256 + m3d::align_up((size_t)num_voxels * sizeof(int), 256) + m3d::align_up(label_blocks(num_voxels) * sizeof(int), 256);
}

M3D_API int m3d_label_components(const void* d_in, int in_bytes, int depth, int height, int width, int connectivity, int32_t* d_labels,
                                 int32_t* d_num, void* d_ws, size_t ws_bytes, void* stream) {
  if (depth <= 0 || height <= 0 || width <= 0) return M3D_EINVAL;
  if (in_bytes != 1 && in_bytes != 2 && in_bytes != 4) return M3D_EINVAL;
  if (connectivity != 6 && connectivity != 18 && connectivity != 26) return M3D_EINVAL;
  const long long V = (long long)depth * height * width;
  if (V >= (1ll << 31)) return M3D_EUNSUPPORTED;                      // parents and labels are int32
  if (!d_in || !d_labels || !d_num || !d_ws) return M3D_EINVAL;
  if (ws_bytes < m3d_label_components_workspace_bytes(V)) return M3D_EWORKSPACE;
  int* parent = (int*)m3d::align_up((size_t)d_ws, 256);
  int* sums = (int*)((char*)parent + m3d::align_up((size_t)V * sizeof(int), 256));
  const int nblocks = (int)label_blocks(V);
  hipStream_t st = m3d::as_stream(stream);
  if (in_bytes == 1) launch_label<uint8_t>(d_in, (int)V, height, width, connectivity, parent, st);
  else if (in_bytes == 2) launch_label<uint16_t>(d_in, (int)V, height, width, connectivity, parent, st);
  else launch_label<uint32_t>(d_in, (int)V, height, width, connectivity, parent, st);
  hipLaunchKernelGGL(lc_flatten, dim3(nblocks), dim3(kT), 0, st, parent, (int)V, sums);
  hipLaunchKernelGGL(lc_scan, dim3(1), dim3(kScanThreads), 0, st, sums, nblocks, d_num);
  hipLaunchKernelGGL(lc_relabel, dim3(grid_for(V, 16384)), dim3(kT), 0, st, (const int*)parent, (const int*)sums, (int)V, d_labels);
  return m3d::check_launch("label_components");
}

M3D_API int m3d_label_counts(const int32_t* d_labels, int64_t num_voxels, int num_labels, int64_t* d_counts, void* stream) {
  if (num_voxels < 0 || num_labels < 0 || !d_counts || (num_voxels && !d_labels)) return M3D_EINVAL;
  hipStream_t st = m3d::as_stream(stream);
  if (hipMemsetAsync(d_counts, 0, ((size_t)num_labels + 1) * sizeof(int64_t), st) != hipSuccess) return m3d::check_launch("label_counts");
  if (num_voxels == 0) return M3D_OK;
  const long long items = (num_voxels + kCountPer - 1) / kCountPer;
  const int grid = grid_for(items, 2048);
  const long long per_block = ((items + grid - 1) / grid + kT - 1) / kT * kT;
  hipLaunchKernelGGL(lcount_kernel, dim3(grid), dim3(kT), 0, st, d_labels, (long long)num_voxels, num_labels, per_block,
                     (unsigned long long*)d_counts);
  return m3d::check_launch("label_counts");
}

M3D_API size_t m3d_paint_spheres_workspace_bytes(int64_t num_voxels) {
  return 256 + (num_voxels <= 0 ? 0 : (size_t)num_voxels * sizeof(unsigned int));
}

M3D_API int m3d_paint_spheres(const int32_t* d_spheres, int num_spheres, int depth, int height, int width, uint16_t* d_volume, void* d_ws,
                              size_t ws_bytes, void* stream) {
  if (num_spheres < 0 || depth <= 0 || height <= 0 || width <= 0) return M3D_EINVAL;
  if (num_spheres > 65535) return M3D_EINVAL;                          // the reference's uint16 volume would wrap silently
  const long long V = (long long)depth * height * width;
  if (V >= (1ll << 31)) return M3D_EUNSUPPORTED;
  if (!d_volume || !d_ws || (num_spheres && !d_spheres)) return M3D_EINVAL;
  if (ws_bytes < m3d_paint_spheres_workspace_bytes(V)) return M3D_EWORKSPACE;
  unsigned int* vol32 = (unsigned int*)m3d::align_up((size_t)d_ws, 256);
  hipStream_t st = m3d::as_stream(stream);
  if (hipMemsetAsync(vol32, 0, (size_t)V * sizeof(unsigned int), st) != hipSuccess) return m3d::check_launch("paint_spheres");
  if (num_spheres) hipLaunchKernelGGL(sphere_paint, dim3(64, num_spheres), dim3(kT), 0, st, d_spheres, depth, height, width, vol32);
  hipLaunchKernelGGL(sphere_narrow, dim3(grid_for(V, 8192)), dim3(kT), 0, st, (const unsigned int*)vol32, V, d_volume);
  return m3d::check_launch("paint_spheres");
}
