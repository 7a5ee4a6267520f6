// evh_plane_components.h -- connected components of the moving-object masks (include/evhip.h states the contract for
// evh_mask_components).  Included by evh_plane.hip inside its unnamed namespace, after the plate entries: it uses their checks
// (Span, need_apart, need_area) and the launch plumbing, and adds kernels of its own only.
//
// Per group of masks that the work buffer holds, on grid.z:
//   k_cc_tile          one workgroup per tile of CC_TW x CC_TH pixels: mask + halo 2r -> LDS, erosion and dilation in LDS, union-find
//                      in LDS; d_labels gets every pixel's tile root as a raster index y*dw + x (background: -1), area gets 0
//   k_cc_merge         one thread per pixel on a tile edge: unions across the edge, atomicMin on roots, every read an agent-scope load
//   k_cc_flatten_roots the pixels whose parent lies in another tile (the tile roots the merge linked) walk to their root and store it
//   k_cc_flatten_area  every pixel walks to its root, now a link or two away, and stores it; area[root] is summed per workgroup for
//                      the root of the workgroup's first pixel, per run of equal roots inside a wave for the others
//   k_cc_count         per chunk of CC_CHUNK pixels the number of kept roots (label == own index, area >= min_area), kept in
//                      ord[first pixel of the chunk]
//   k_cc_scan          one workgroup per mask: the chunk counts become exclusive prefixes in place; d_nobjects = the total
//   k_cc_number        ord[i] = number of the kept root i (else 0); a numbered root starts its row of the table
//   k_cc_relabel       d_labels = ord[root]; box and sums go to the table by atomics, summed per workgroup and per run likewise
// Every link points to a strictly smaller raster index (a root to itself), so a component's root is its first pixel in raster
// order and every walk ends.  No workgroup waits for another: ordering comes from the kernel boundaries alone.  All sums are
// integers: the result does not depend on the order of arrival.

constexpr int CC_TW = EVH_COMPONENTS_TILE_W, CC_TH = EVH_COMPONENTS_TILE_H, CC_TILE = CC_TW * CC_TH, CC_MAXR = 3;
constexpr int CC_PPT = 8, CC_SPAN = 256 * CC_PPT;  // pixels per thread and per workgroup of the two passes that sum (area; box and centre)
constexpr int CC_CHUNK = 1024;                 // pixels per workgroup of the count and number passes: 4 per thread
constexpr int64_t CC_GROUP_BYTES = 1 << 28;    // evh_mask_components_work_bytes asks for no more than this, or one mask

// ---- union-find in LDS: P[i] = i for a root, a smaller index for a linked pixel, -1 for background -------------------------------
__device__ __forceinline__ int cc_lds_load(const int* P, int a) {
  return __hip_atomic_load(P + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int cc_lds_root(const int* P, int a) {
  int p;
  while ((p = cc_lds_load(P, a)) != a) a = p;          // ends: a link points to a strictly smaller index
  return a;
}
__device__ __forceinline__ void cc_lds_unite(int* P, int a, int b) {
  a = cc_lds_root(P, a); b = cc_lds_root(P, b);
  while (a != b) {                                     // ends: the larger of (a, b) is replaced by a strictly smaller index
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(P + a, b);               // a -> min(P[a], b): never upwards
    if (old == a) break;                               // a was a root and now hangs under b
    a = old;                                           // a hung under old: old and b are still to be joined
  }
}

// ---- union-find over d_labels: the value at raster index i is the parent of i -----------------------------------------------------
struct CcLabels { int32_t* p; int64_t row_stride; int dw; };
__device__ __forceinline__ int32_t* cc_at(const CcLabels& L, int i) {
  if (L.row_stride == L.dw) return L.p + i;
  const int y = i / L.dw;
  return L.p + (y * L.row_stride + (i - y * L.dw));
}
// agent scope: a plain load may stay stale in this CU's cache while another XCD's atomicMin has lowered the value
__device__ __forceinline__ int cc_load(const CcLabels& L, int i) {
  return __hip_atomic_load(cc_at(L, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int cc_root(const CcLabels& L, int a) {
  int p;
  while ((p = cc_load(L, a)) != a) a = p;              // ends: a link points to a strictly smaller index
  return a;
}
__device__ __forceinline__ void cc_unite(const CcLabels& L, int a, int b) {
  const int a0 = a, b0 = b;
  a = cc_root(L, a); b = cc_root(L, b);
  // the walked paths shortened for whoever comes next: a link may always move to a further ancestor, never upwards
  if (a != a0) atomicMin(cc_at(L, a0), a);
  if (b != b0) atomicMin(cc_at(L, b0), b);
  while (a != b) {                                     // ends: the larger of (a, b) is replaced by a strictly smaller index
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(cc_at(L, a), b);
    if (old == a) break;
    a = old;
  }
}

// The flatten passes walk with loads that may be served from a cache: between kernel boundaries a link only ever moves to a
// further ancestor, so a stale value still lies on the pixel's path.
__device__ __forceinline__ int cc_load_cached(const CcLabels& L, int i) {
  return __hip_atomic_load(cc_at(L, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int cc_root_cached(const CcLabels& L, int a) {
  int p;
  while ((p = cc_load_cached(L, a)) != a) a = p;       // ends: a link points to a strictly smaller index
  return a;
}

// The runs of equal keys along a wave's 64 consecutive raster pixels: the length of the run for its first lane, 0 for every
// other lane.  `cut` starts a new run (the first pixel of a row, where a run must stay on one row).  All 64 lanes call it.
__device__ __forceinline__ int cc_run_length(int key, bool cut) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(key, 1, 64);
  const bool head = lane == 0 || prev != key || cut;
  const unsigned long long heads = __ballot(head);
  if (!head) return 0;
  const unsigned long long after = (heads >> lane) >> 1;
  return after ? __builtin_ctzll(after) + 1 : 64 - lane;
}

__global__ __launch_bounds__(256) void k_cc_tile(const uint8_t* __restrict__ mask, int64_t mask_stride, int64_t mask_img_stride, int m0,
                                                 int dw, int dh, int conn8, int r, int32_t* __restrict__ labels, int64_t label_stride,
                                                 int64_t label_img_stride, int32_t* __restrict__ area, unsigned tiles_across) {
  __shared__ uint8_t raw[(CC_TH + 4 * CC_MAXR) * (CC_TW + 4 * CC_MAXR)];     // the mask with a halo of 2r, 0 outside the canvas
  __shared__ uint8_t ero[(CC_TH + 2 * CC_MAXR) * (CC_TW + 2 * CC_MAXR)];     // the erosion with a halo of r
  __shared__ int P[CC_TILE];
  const unsigned tile_y = blockIdx.x / tiles_across;      // the tiles on grid.x: a canvas may be a million tiles high
  const int tid = threadIdx.x, tx0 = (int)(blockIdx.x - tile_y * tiles_across) * CC_TW, ty0 = (int)tile_y * CC_TH;
  const uint8_t* M = mask + (int64_t)(m0 + (int)blockIdx.z) * mask_img_stride;
  const int rw = CC_TW + 4 * r, rh = CC_TH + 4 * r, ew = CC_TW + 2 * r, eh = CC_TH + 2 * r;
  for (int i = tid; i < rw * rh; i += 256) {           // ends: i grows to rw * rh
    const int ly = i / rw, lx = i - ly * rw, x = tx0 + lx - 2 * r, y = ty0 + ly - 2 * r;
    raw[i] = (x >= 0 && x < dw && y >= 0 && y < dh) ? (M[y * mask_stride + x] != 0) : 0;
  }
  __syncthreads();
  if (r > 0) {
    for (int i = tid; i < ew * eh; i += 256) {         // ends: i grows to ew * eh
      const int ly = i / ew, lx = i - ly * ew;
      int all = 1;
      for (int j = 0; j <= 2 * r; j++)                 // ends: j grows to 2r
        for (int k = 0; k <= 2 * r; k++) all &= raw[(ly + j) * rw + lx + k];      // ends: k grows to 2r
      ero[i] = (uint8_t)all;
    }
    __syncthreads();
  }
  for (int i = tid; i < CC_TILE; i += 256) {           // ends: i grows to CC_TILE
    const int ly = i / CC_TW, lx = i - ly * CC_TW;
    int fg = 0;
    if (r == 0) fg = raw[ly * rw + lx];
    else
      for (int j = 0; j <= 2 * r; j++)                 // ends: j grows to 2r
        for (int k = 0; k <= 2 * r; k++) fg |= ero[(ly + j) * ew + lx + k];       // ends: k grows to 2r
    P[i] = fg ? i : -1;
  }
  __syncthreads();
  for (int i = tid; i < CC_TILE; i += 256) {           // ends: i grows to CC_TILE
    if (cc_lds_load(P, i) < 0) continue;
    const int ly = i / CC_TW, lx = i - ly * CC_TW;
    if (lx > 0 && cc_lds_load(P, i - 1) >= 0) cc_lds_unite(P, i, i - 1);
    if (ly > 0) {
      if (cc_lds_load(P, i - CC_TW) >= 0) cc_lds_unite(P, i, i - CC_TW);
      else if (conn8) {                                // with the pixel above set, both diagonals hang on it already
        if (lx > 0 && cc_lds_load(P, i - CC_TW - 1) >= 0) cc_lds_unite(P, i, i - CC_TW - 1);
        if (lx < CC_TW - 1 && cc_lds_load(P, i - CC_TW + 1) >= 0) cc_lds_unite(P, i, i - CC_TW + 1);
      }
    }
  }
  __syncthreads();
  int32_t* L = labels + (int64_t)(m0 + (int)blockIdx.z) * label_img_stride;
  int32_t* A = area + (int64_t)blockIdx.z * ((int64_t)dw * dh);
  for (int i = tid; i < CC_TILE; i += 256) {           // ends: i grows to CC_TILE
    const int ly = i / CC_TW, lx = i - ly * CC_TW, x = tx0 + lx, y = ty0 + ly;
    if (x >= dw || y >= dh) continue;
    int v = -1;
    if (cc_lds_load(P, i) >= 0) {
      const int root = cc_lds_root(P, i), ry = root / CC_TW;
      v = (ty0 + ry) * dw + tx0 + (root - ry * CC_TW);
    }
    L[y * label_stride + x] = v;
    A[y * dw + x] = 0;
  }
}

// nv = (tiles across - 1) * dh pixels left of which a tile ends, then (tiles down - 1) * dw pixels above which one ends
__global__ __launch_bounds__(256) void k_cc_merge(int32_t* labels, int64_t label_stride, int64_t label_img_stride, int m0, int dw, int dh,
                                                  int conn8, int nv, int total) {
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const CcLabels L = {labels + (int64_t)(m0 + (int)blockIdx.z) * label_img_stride, label_stride, dw};
  int x, y;
  const bool vertical = t < nv;
  if (vertical) {
    const int c = t / dh;
    y = t - c * dh; x = (c + 1) * CC_TW;
  } else {
    t -= nv;
    const int rr = t / dw;
    x = t - rr * dw; y = (rr + 1) * CC_TH;
  }
  const int me = y * dw + x;
  if (cc_load(L, me) < 0) return;
  auto join = [&](int nx, int ny) {
    const int other = ny * dw + nx;
    if (cc_load(L, other) >= 0) cc_unite(L, me, other);
  };
  if (vertical) {
    join(x - 1, y);
    if (conn8) {
      if (y > 0) join(x - 1, y - 1);
      if (y + 1 < dh) join(x - 1, y + 1);
    }
  } else {
    join(x, y - 1);
    if (conn8) {
      if (x > 0) join(x - 1, y - 1);
      if (x + 1 < dw) join(x + 1, y - 1);
    }
  }
}

// After the merge a pixel that was not its tile's root still points to that root, inside its own tile: only roots were ever
// linked.  So the long walks are left to the tile roots (a parent outside the pixel's tile, or the pixel itself) ...
__global__ __launch_bounds__(256) void k_cc_flatten_roots(int32_t* labels, int64_t label_stride, int64_t label_img_stride, int m0, int dw,
                                                          int npix) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)npix) return;
  const CcLabels L = {labels + (int64_t)(m0 + (int)blockIdx.z) * label_img_stride, label_stride, dw};
  const int p = cc_load_cached(L, (int)i);
  if (p < 0 || p == (int)i) return;
  const int y = (int)i / dw, x = (int)i - y * dw, py = p / dw, px = p - py * dw;
  if (px / CC_TW == x / CC_TW && py / CC_TH == y / CC_TH) return;
  // whoever walks through this pixel meanwhile reads its old parent or its root: both lie on its path
  __hip_atomic_store(cc_at(L, (int)i), cc_root_cached(L, p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// ... and every other pixel finds its root one link behind its tile root.
// The sums of the two reducing passes, workgroup first (a mask that is one component would otherwise send every run of every wave
// to one address): a workgroup takes CC_SPAN consecutive raster pixels, CC_PPT per thread.  Its LEADER is the key of its first
// pixel that has one; the leader's pixels are summed in registers and then in LDS, one set of global atomics per workgroup.  The
// pixels of other keys go by runs inside a wave, as before.
__global__ __launch_bounds__(256) void k_cc_flatten_area(int32_t* labels, int64_t label_stride, int64_t label_img_stride, int m0, int dw,
                                                         int npix, int32_t* area) {
  __shared__ int s_first, s_leader, s_count;
  const int tid = threadIdx.x;
  const unsigned i0 = blockIdx.x * (unsigned)CC_SPAN;
  const CcLabels L = {labels + (int64_t)(m0 + (int)blockIdx.z) * label_img_stride, label_stride, dw};
  if (tid == 0) { s_first = INT_MAX; s_leader = -1; s_count = 0; }
  __syncthreads();
  int root[CC_PPT];
  int mine = INT_MAX;
#pragma unroll
  for (int k = 0; k < CC_PPT; k++) {                   // ends: k grows to CC_PPT
    const unsigned i = i0 + k * 256 + tid;
    root[k] = -2;                                      // past the mask: a key no pixel has
    if (i < (unsigned)npix) {
      int r = cc_load_cached(L, (int)i);
      if (r >= 0) {
        r = cc_root_cached(L, r);
        __hip_atomic_store(cc_at(L, (int)i), r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      root[k] = r;
    }
    if (root[k] >= 0 && mine == INT_MAX) mine = k * 256 + tid;
  }
  if (mine != INT_MAX) atomicMin(&s_first, mine);
  __syncthreads();
  const int first = s_first;
#pragma unroll
  for (int k = 0; k < CC_PPT; k++)                     // ends: k grows to CC_PPT
    if (first == k * 256 + tid) s_leader = root[k];
  __syncthreads();
  const int leader = s_leader;                         // -1: the span holds background only
  int32_t* A = area + (int64_t)blockIdx.z * npix;
  int count = 0;
#pragma unroll
  for (int k = 0; k < CC_PPT; k++) {                   // ends: k grows to CC_PPT
    const bool led = root[k] >= 0 && root[k] == leader;
    count += led;
    const int len = cc_run_length(led ? -3 : root[k], false);
    if (len > 0 && root[k] >= 0 && !led) atomicAdd(A + root[k], len);
  }
  if (count) atomicAdd(&s_count, count);
  __syncthreads();
  if (tid == 0 && s_count) atomicAdd(A + leader, s_count);
}

__device__ __forceinline__ bool cc_kept(const CcLabels& L, const int32_t* area, unsigned i, int npix, int min_area) {
  return i < (unsigned)npix && *cc_at(L, (int)i) == (int)i && area[i] >= min_area;
}

__global__ __launch_bounds__(256) void k_cc_count(const int32_t* labels, int64_t label_stride, int64_t label_img_stride, int m0, int dw,
                                                  int npix, const int32_t* area, int min_area, int32_t* ord) {
  const CcLabels L = {const_cast<int32_t*>(labels) + (int64_t)(m0 + (int)blockIdx.z) * label_img_stride, label_stride, dw};
  const int64_t base = (int64_t)blockIdx.z * npix;
  const unsigned i0 = blockIdx.x * (unsigned)CC_CHUNK;
  int n = 0;
  for (int k = 0; k < CC_CHUNK / 256; k++)             // ends: k grows to 4
    n += __syncthreads_count(cc_kept(L, area + base, i0 + k * 256 + threadIdx.x, npix, min_area));
  if (threadIdx.x == 0) ord[base + i0] = n;
}

__global__ __launch_bounds__(256) void k_cc_scan(int32_t* ord, int npix, int nchunks, int m0, int32_t* nobjects) {
  __shared__ int part[256];
  __shared__ int carry;
  int32_t* O = ord + (int64_t)blockIdx.x * npix;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int c0 = 0; c0 < nchunks; c0 += 256) {          // ends: c0 grows to nchunks
    const int c = c0 + tid;
    const int v = c < nchunks ? O[(int64_t)c * CC_CHUNK] : 0;
    part[tid] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                // ends: d doubles to 256
      const int add = tid >= d ? part[tid - d] : 0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    const int before = carry + part[tid] - v;
    if (c < nchunks) O[(int64_t)c * CC_CHUNK] = before;
    __syncthreads();
    if (tid == 255) carry += part[255];
    __syncthreads();
  }
  if (tid == 0) nobjects[m0 + blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void k_cc_number(const int32_t* labels, int64_t label_stride, int64_t label_img_stride, int m0, int dw,
                                                   int npix, const int32_t* area, int min_area, int32_t* ord, evh_component* objects,
                                                   int max_objects) {
  __shared__ int waves[4];
  const CcLabels L = {const_cast<int32_t*>(labels) + (int64_t)(m0 + (int)blockIdx.z) * label_img_stride, label_stride, dw};
  const int64_t base = (int64_t)blockIdx.z * npix;
  const unsigned i0 = blockIdx.x * (unsigned)CC_CHUNK;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int before = ord[base + i0];                         // the kept roots in front of this chunk; its slot is rewritten below
  __syncthreads();
  for (int k = 0; k < CC_CHUNK / 256; k++) {           // ends: k grows to 4
    const unsigned i = i0 + k * 256 + threadIdx.x;
    const bool kept = cc_kept(L, area + base, i, npix, min_area);
    const unsigned long long votes = __ballot(kept);
    if (lane == 0) waves[wave] = __popcll(votes);
    __syncthreads();
    int mine = before + __popcll(votes & ((1ull << lane) - 1));
    for (int w = 0; w < wave; w++) mine += waves[w];   // ends: w grows to wave < 4
    const int all = waves[0] + waves[1] + waves[2] + waves[3];
    __syncthreads();
    before += all;
    if (i < (unsigned)npix) {
      const int number = kept ? mine + 1 : 0;
      ord[base + i] = number;
      if (kept && number <= max_objects) {
        const int y = (int)i / dw;
        evh_component o;
        o.x0 = INT_MAX; o.y0 = y; o.x1 = -1; o.y1 = y; o.area = area[base + i]; o.first = (int)i; o.sx = 0; o.sy = 0;
        objects[(int64_t)(m0 + (int)blockIdx.z) * max_objects + number - 1] = o;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_cc_relabel(int32_t* labels, int64_t label_stride, int64_t label_img_stride, int m0, int dw,
                                                    int npix, const int32_t* ord, evh_component* objects, int max_objects) {
  __shared__ int s_first, s_leader, s_x0, s_x1, s_y1;
  __shared__ unsigned long long s_sx, s_sy;
  const int tid = threadIdx.x;
  const unsigned i0 = blockIdx.x * (unsigned)CC_SPAN;
  const CcLabels L = {labels + (int64_t)(m0 + (int)blockIdx.z) * label_img_stride, label_stride, dw};
  if (tid == 0) { s_first = INT_MAX; s_leader = 0; s_x0 = INT_MAX; s_x1 = -1; s_y1 = -1; s_sx = 0; s_sy = 0; }
  __syncthreads();
  int key[CC_PPT], x[CC_PPT], y[CC_PPT];
  int mine = INT_MAX;
#pragma unroll
  for (int k = 0; k < CC_PPT; k++) {                   // ends: k grows to CC_PPT
    const unsigned i = i0 + k * 256 + tid;
    key[k] = -1; x[k] = 0; y[k] = 0;
    if (i < (unsigned)npix) {
      y[k] = (int)i / dw; x[k] = (int)i - y[k] * dw;
      int32_t* at = L.p + (y[k] * label_stride + x[k]);
      const int root = *at;                             // only this thread reads or writes this element here
      const int number = root >= 0 ? ord[(int64_t)blockIdx.z * npix + root] : 0;
      *at = number;
      key[k] = number > 0 && number <= max_objects ? number : 0;
    }
    if (key[k] > 0 && mine == INT_MAX) mine = k * 256 + tid;
  }
  if (mine != INT_MAX) atomicMin(&s_first, mine);
  __syncthreads();
  const int first = s_first;
#pragma unroll
  for (int k = 0; k < CC_PPT; k++)                     // ends: k grows to CC_PPT
    if (first == k * 256 + tid) s_leader = key[k];
  __syncthreads();
  const int leader = s_leader;                         // 0: no pixel of the span goes to the table
  evh_component* table = objects + (int64_t)(m0 + (int)blockIdx.z) * max_objects;
  int x0 = INT_MAX, x1 = -1, y1 = -1;
  unsigned long long sx = 0, sy = 0;
#pragma unroll
  for (int k = 0; k < CC_PPT; k++) {                   // ends: k grows to CC_PPT
    const bool led = key[k] > 0 && key[k] == leader;
    if (led) {
      x0 = min(x0, x[k]); x1 = max(x1, x[k]); y1 = max(y1, y[k]);
      sx += (unsigned long long)x[k]; sy += (unsigned long long)y[k];
    }
    const int len = cc_run_length(led ? 0 : key[k], x[k] == 0);
    if (len > 0 && key[k] > 0 && !led) {
      evh_component* o = table + (key[k] - 1);
      const unsigned long long n = (unsigned long long)len;
      atomicMin(&o->x0, x[k]);
      atomicMax(&o->x1, x[k] + len - 1);
      atomicMax(&o->y1, y[k]);
      atomicAdd(reinterpret_cast<unsigned long long*>(&o->sx), n * (unsigned long long)x[k] + n * (n - 1) / 2);
      atomicAdd(reinterpret_cast<unsigned long long*>(&o->sy), n * (unsigned long long)y[k]);
    }
  }
  if (x1 >= 0) {
    atomicMin(&s_x0, x0); atomicMax(&s_x1, x1); atomicMax(&s_y1, y1);
    atomicAdd(&s_sx, sx); atomicAdd(&s_sy, sy);
  }
  __syncthreads();
  if (tid == 0 && s_x1 >= 0) {
    evh_component* o = table + (leader - 1);
    atomicMin(&o->x0, s_x0);
    atomicMax(&o->x1, s_x1);
    atomicMax(&o->y1, s_y1);
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->sx), s_sx);
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->sy), s_sy);
  }
}

// ---- the entry ------------------------------------------------------------------------------------------------------------------------
// 0 for sizes the entry refuses; else 8 bytes per pixel for as many masks as CC_GROUP_BYTES holds, at least one
size_t components_work_bytes(int dw, int dh, int nmasks) {
  if (dw < 1 || dh < 1 || nmasks < 0 || nmasks > 65535 || (int64_t)dw * dh > INT_MAX) return 0;
  const int64_t per = (int64_t)dw * dh * 8;
  return (size_t)(per * std::min<int64_t>(nmasks, std::max<int64_t>(1, CC_GROUP_BYTES / per)));
}
struct ComponentsArgs {
  const char* who; const uint8_t* mask; int nmasks, dw, dh; int64_t mask_stride, mask_img_stride; int connectivity, open_radius, min_area;
  int32_t* labels; int64_t label_stride, label_img_stride; evh_component* objects; int max_objects; int32_t* nobjects; void* work;
  size_t work_bytes;
  bool idle() const { return nmasks == 0; }
};
int check(evh_ctx* c, const ComponentsArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (!A.mask || !A.labels || !A.nobjects || !A.work) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (A.max_objects < 0 || (!A.objects && A.max_objects > 0))
    return evh_fail(c, EVH_ERR_INVALID, W + "max_objects must not be negative, and d_objects may be NULL only when it is 0");
  if (A.connectivity != 4 && A.connectivity != 8) return evh_fail(c, EVH_ERR_INVALID, W + "connectivity must be 4 or 8");
  if (A.open_radius < 0 || A.open_radius > CC_MAXR) return evh_fail(c, EVH_ERR_INVALID, W + "open_radius must lie in 0..3");
  if (A.min_area < 1) return evh_fail(c, EVH_ERR_INVALID, W + "min_area must be at least 1");
  if (A.dw < 1 || A.dh < 1 || A.nmasks < 0) return evh_fail(c, EVH_ERR_INVALID, W + "empty canvas or negative nmasks");
  if (int rc = need_area(c, W, "dw * dh", A.dw, A.dh)) return rc;
  if (A.nmasks > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 masks per call");
  const int64_t picture = (A.dh - 1) * A.mask_stride + A.dw, sheet = (A.dh - 1) * A.label_stride + A.dw;
  if (A.mask_stride < A.dw || (A.nmasks > 1 && A.mask_img_stride < picture))
    return evh_fail(c, EVH_ERR_INVALID, W + "mask stride smaller than a row / picture");
  if (A.label_stride < A.dw || (A.nmasks > 1 && A.label_img_stride < sheet))
    return evh_fail(c, EVH_ERR_INVALID, W + "label stride smaller than a row / picture");
  if (((uintptr_t)A.labels | (uintptr_t)A.nobjects | (uintptr_t)A.work) & 3)
    return evh_fail(c, EVH_ERR_INVALID, W + "d_labels, d_nobjects and d_work must be 4-byte aligned");
  if ((uintptr_t)A.objects & 7) return evh_fail(c, EVH_ERR_INVALID, W + "d_objects must be 8-byte aligned");
  if (A.work_bytes < components_work_bytes(A.dw, A.dh, A.nmasks))
    return evh_fail(c, EVH_ERR_INVALID, W + "work_bytes below evh_mask_components_work_bytes");
  if (A.nmasks == 0) return EVH_SUCCESS;
  const int64_t last = A.nmasks - 1;
  const Span outs[4] = {{A.labels, (sheet + last * A.label_img_stride) * 4, "d_labels"},
                        {A.objects, (int64_t)A.nmasks * A.max_objects * (int64_t)sizeof(evh_component), "d_objects"},
                        {A.nobjects, (int64_t)A.nmasks * 4, "d_nobjects"}, {A.work, (int64_t)A.work_bytes, "d_work"}};
  const Span ins[1] = {{A.mask, picture + last * A.mask_img_stride, "d_mask"}};
  return need_apart(c, W, outs, ins);
}
// the eight launches above (six for a canvas of one tile), once per group of masks that d_work holds (1 <= nmasks <= 65535)
int launch(evh_ctx* c, const ComponentsArgs& A) {
  const int npix = A.dw * A.dh, conn8 = A.connectivity == 8;
  const int64_t per = (int64_t)npix * 8;
  const int group = (int)std::min<int64_t>(A.nmasks, (int64_t)(A.work_bytes / (size_t)per));
  int32_t* area = static_cast<int32_t*>(A.work);
  int32_t* ord = area + (int64_t)group * npix;
  const unsigned tx = (A.dw + CC_TW - 1) / CC_TW, ty = (A.dh + CC_TH - 1) / CC_TH;
  const int nv = (int)(tx - 1) * A.dh, edge = nv + (int)(ty - 1) * A.dw;
  const unsigned blocks = ((unsigned)npix + 255u) / 256u, chunks = ((unsigned)npix + CC_CHUNK - 1) / CC_CHUNK,
                 spans = ((unsigned)npix + CC_SPAN - 1) / CC_SPAN;
  for (int m0 = 0; m0 < A.nmasks; m0 += group) {
    const unsigned g = (unsigned)std::min(group, A.nmasks - m0);
    hipLaunchKernelGGL(k_cc_tile, dim3(tx * ty, 1, g), dim3(256), 0, c->stream, A.mask, A.mask_stride, A.mask_img_stride, m0, A.dw, A.dh,
                       conn8, A.open_radius, A.labels, A.label_stride, A.label_img_stride, area, tx);
    if (edge > 0)
      hipLaunchKernelGGL(k_cc_merge, dim3((edge + 255) / 256, 1, g), dim3(256), 0, c->stream, A.labels, A.label_stride,
                         A.label_img_stride, m0, A.dw, A.dh, conn8, nv, edge);
    if (edge > 0)
      hipLaunchKernelGGL(k_cc_flatten_roots, dim3(blocks, 1, g), dim3(256), 0, c->stream, A.labels, A.label_stride, A.label_img_stride,
                         m0, A.dw, npix);
    hipLaunchKernelGGL(k_cc_flatten_area, dim3(spans, 1, g), dim3(256), 0, c->stream, A.labels, A.label_stride, A.label_img_stride, m0,
                       A.dw, npix, area);
    hipLaunchKernelGGL(k_cc_count, dim3(chunks, 1, g), dim3(256), 0, c->stream, A.labels, A.label_stride, A.label_img_stride, m0, A.dw,
                       npix, area, A.min_area, ord);
    hipLaunchKernelGGL(k_cc_scan, dim3(g), dim3(256), 0, c->stream, ord, npix, (int)chunks, m0, A.nobjects);
    hipLaunchKernelGGL(k_cc_number, dim3(chunks, 1, g), dim3(256), 0, c->stream, A.labels, A.label_stride, A.label_img_stride, m0, A.dw,
                       npix, area, A.min_area, ord, A.objects, A.max_objects);
    hipLaunchKernelGGL(k_cc_relabel, dim3(spans, 1, g), dim3(256), 0, c->stream, A.labels, A.label_stride, A.label_img_stride, m0, A.dw,
                       npix, ord, A.objects, A.max_objects);
    if (int rc = launched(c)) return rc;
  }
  return EVH_SUCCESS;
}
