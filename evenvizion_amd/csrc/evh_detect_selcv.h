// evh_detect_selcv.h -- internal to evh_detect.hip (stage 4 of 5): selection in the reference's key-point order
#pragma once
#include "evh_detect_fast.h"
#include "evh_detect_select.h"
namespace {
// K4, reference order (EVH_ORDER_OPENCV, the default).  KeyPointsFilter::retainBest (features2d/src/keypoint.cpp) is
//     std::nth_element(begin, begin + n, end, response-greater); amb = kp[n - 1].response;
//     new_end = std::partition(begin + n, end, response >= amb); resize(new_end - begin)
// and both calls PERMUTE the vector: the order ORB hands its key points over in -- hence the order of the matches, of the
// rows given to RANSAC, hence which minimal samples its random generator draws -- is the order libstdc++'s introselect and
// partition leave behind, and with ties at the cut even the surviving SET depends on it (position n - 1 holds an arbitrary
// member of the best n).  The reference's own recorded run agrees with this order and with no other
// (tests/test_capture_golden.py), so the order is part of the operator.  k_select_cv runs the same algorithms on the same
// sequence (FAST corners of a level in row-major order), with every pass over the data done by the whole workgroup:
//   * Hoare's unguarded partition = pair the k-th element from the left that is not "before" the pivot with the k-th from
//     the right that is not "after" it while the former lies left of the latter; the pairs are independent, so the two
//     stopper lists are built by ranking, the number of pairs by a search, the swaps in parallel; the cut follows from the
//     first unpaired stoppers.  std::partition is the same with a predicate.
//   * the row-major sequence is made before k_select_cv starts, by two launches of their own (k_cv_band_base, k_cv_place at
//     the end of this file): pure data movement, shaped for the memory system and not for the selection's one workgroup per level.
// What stays sequential is what libstdc++ does per round in O(1): the median-of-three pivot and the final insertion sort.
// The kernel is bound by dependent memory round trips and barriers, not by bytes or arithmetic, so every pass is shaped to
// have few of them: loads that do not depend on one another, one exchange between the waves per partition pass (cv_partition),
// list entries stored only where a pair can use them, short ranges and (where they fit) whole short levels in LDS.
struct SelCvArgs {
  SelectArgs s;
  unsigned long long* seq;   // [nframes][cand_frame_entries]  stage 2: Harris key << 32 | packed candidate
  uint32_t* seq32;           // [nframes][cand_frame_entries]  stage 1: the candidates themselves (key = FAST score = top byte)
  uint32_t* lpos;            // [nframes][cand_frame_entries]  left-stopper positions, ascending
  uint32_t* rpos;            // [nframes][cand_frame_entries]  right-stopper positions, ascending
  const uint32_t* tdesc;     // [nframes][total_tiles][8] tile burst descriptors written by k_fast
  int total_tiles;
  int* band;                 // [nframes][band_frame_entries] k_cv_band_base: corners before each band of its level, then the 8 level totals
  int band_frame_entries;
  int band_start[EVH_NLEVELS];   // first band of a level among the frame's bands (a band = one row of FAST tiles)
  int nbands;                // bands of a frame, all levels
  int heap_cap;              // entries of the dynamic LDS heap (>= 2 * largest quota + 1)
  int phase_limit;           // profiling aid: 1 = stop after the row-major sequence, 2 = after the first retainBest, 0 = all
};

struct CvLds {
  int wsumL[16], wsumR[16];   // per-wave totals; k_select_cv runs 4 waves (256 threads, its launch bounds), the arrays leave room for 16
  int bc[16];
};

#define CV_NOPOS 0x7FFFFFFF

// exclusive prefix of (a, b) over the threads of the workgroup (blockDim.x = 64 * NW); totals come back in ta / tb.  Two barriers.
__device__ __forceinline__ void cv_scan2(CvLds& S, int a, int b, int& ea, int& eb, int& ta, int& tb) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int ia = a, ib = b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int ua = __shfl_up(ia, o), ub = __shfl_up(ib, o);
    if (lane >= o) { ia += ua; ib += ub; }
  }
  if (lane == 63) { S.wsumL[wv] = ia; S.wsumR[wv] = ib; }
  __syncthreads();
  int ba = 0, bb = 0;
  ta = 0; tb = 0;
  const int nw = (int)blockDim.x >> 6;
  for (int w = 0; w < nw; w++) {
    const int l_ = S.wsumL[w], r_ = S.wsumR[w];
    if (w < wv) { ba += l_; bb += r_; }
    ta += l_; tb += r_;
  }
  ea = ba + ia - a;
  eb = bb + ib - b;
  __syncthreads();
}

// Partition pass over a[lo, hi).  MODE 0: Hoare around the pivot key p (left stoppers key <= p, right stoppers key >= p),
// returns the cut.  MODE 1: std::partition with the predicate key >= p (left stoppers !pred, right stoppers pred), returns
// the position of the first element of the false group.  EP / LP: element and position-list pointers (global memory with
// 32-bit positions, or the LDS copy of a short range with 16-bit positions).
// element = key << 32 | candidate (64-bit: the Harris stage) or the 32-bit candidate itself, whose top byte is the FAST score
__device__ __forceinline__ uint32_t cv_key(unsigned long long e) { return (uint32_t)(e >> 32); }
__device__ __forceinline__ uint32_t cv_key(uint32_t e) { return cand_score(e); }
template <class E>
__device__ __forceinline__ bool cv_gt(E x, E y) { return cv_key(x) > cv_key(y); }

// How a pass walks memory: every wave owns one contiguous segment of the range and sweeps it in steps of CV_WSTEP elements
// (lane L of step element e takes base + 64 e + L: coalesced, and no load depends on an earlier step).
//   sweep 1 counts the stoppers of the segment (ballots only); ONE exchange of the wave totals over LDS gives cntL, cntR and
//           every wave's first rank -- one barrier per pass, not two per 1024 elements;
//   sweep 2 reads the segment again and stores only the list entries that can pair: at most K = min(cntL, cntR) pairs swap,
//           so the left list is needed up to rank K (rank K decides the cut) and the right list for its LAST K entries.  The
//           right list is therefore kept reversed (rrev[k] = k-th right stopper from the right) and built by a sweep from the
//           segment's end; each direction stops as soon as the wave's ranks have passed K.  The tail std::partition of
//           retainBest (K = the few ties at the cut) stores next to nothing, and nothing at all when cntR == 0.
#define CV_EPT 8                    // elements per lane and wave step: eight loads in flight per lane
#define CV_WSTEP (64 * CV_EPT)      // elements per wave step
__device__ __forceinline__ int cv_lanes_below(unsigned long long bal) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

template <int MODE, class EP, class LP>
__device__ __forceinline__ int cv_partition(EP a, int lo, int hi, uint32_t p, LP lpos, LP rrev, CvLds& S) {
  typedef typename std::remove_pointer<LP>::type PT;
  typedef typename std::remove_pointer<EP>::type E;
  const int tid = threadIdx.x, NT = (int)blockDim.x, NW = NT >> 6, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // the segment bounds and the step loops are the wave's, not the lane's
  const int seg = (hi - lo + NW - 1) / NW;
  const int s0 = min(hi, lo + wv * seg), s1 = min(hi, s0 + seg);   // this wave's segment
  auto is_left = [&](uint32_t key) { return MODE == 0 ? key <= p : key < p; };
  int cl = 0, cr = 0;
  // (the loads of a step are issued together, into key[]: next to the ballots the compiler waits for them one by one)
  for (int b = s0; b < s1; b += CV_WSTEP) {
    uint32_t key[CV_EPT];
#pragma unroll
    for (int e = 0; e < CV_EPT; e++) key[e] = cv_key(a[min(b + 64 * e + lane, s1 - 1)]);
#pragma unroll
    for (int e = 0; e < CV_EPT; e++) {
      const int i = b + 64 * e + lane;
      cl += __popcll(__ballot(i < s1 && is_left(key[e])));
      cr += __popcll(__ballot(i < s1 && key[e] >= p));
    }
  }
  if (lane == 0) { S.wsumL[wv] = cl; S.wsumR[wv] = cr; }
  __syncthreads();
  int cntL = 0, cntR = 0, runL = 0, runR = 0;   // run*: left stoppers in earlier waves, right stoppers in later ones
  for (int w = 0; w < NW; w++) {
    const int l_ = S.wsumL[w], r_ = S.wsumR[w];
    cntL += l_; cntR += r_;
    if (w < wv) runL += l_;
    if (w > wv) runR += r_;
  }
  const int K = min(cntL, cntR);
  if (MODE == 1 && K == 0) {   // nothing can swap
    __syncthreads();           // the wave totals are free
    return lo + cntR;
  }
  const int KL = MODE == 0 ? min(cntL, K + 1) : K;
  for (int b = s0; b < s1 && runL < KL; b += CV_WSTEP) {
    uint32_t key[CV_EPT];
#pragma unroll
    for (int e = 0; e < CV_EPT; e++) key[e] = cv_key(a[min(b + 64 * e + lane, s1 - 1)]);
#pragma unroll
    for (int e = 0; e < CV_EPT; e++) {
      const int i = b + 64 * e + lane;
      const bool st = i < s1 && is_left(key[e]);
      const unsigned long long bal = __ballot(st);
      const int rank = runL + cv_lanes_below(bal);
      if (st && rank < KL) lpos[rank] = (PT)i;
      runL += __popcll(bal);
    }
  }
  for (int t = s1 - 1; t >= s0 && runR < K; t -= CV_WSTEP) {   // from the right: lane 0 takes the last element
    uint32_t key[CV_EPT];
#pragma unroll
    for (int e = 0; e < CV_EPT; e++) key[e] = cv_key(a[max(t - 64 * e - lane, s0)]);
#pragma unroll
    for (int e = 0; e < CV_EPT; e++) {
      const int i = t - 64 * e - lane;
      const bool st = i >= s0 && key[e] >= p;
      const unsigned long long bal = __ballot(st);
      const int rank = runR + cv_lanes_below(bal);
      if (st && rank < K) rrev[rank] = (PT)i;
      runR += __popcll(bal);
    }
  }
  __syncthreads();   // lists complete
  // number of pairs: the largest m with L[k] < R[k] for all k < m (monotone), by NT-way search; R[k] = rrev[k]
  int lo_k = 0, hi_k = K;   // invariant: pairs [0, lo_k) swap, pairs [hi_k, K) do not
  while (hi_k > lo_k) {
    const int span = hi_k - lo_k;
    const int step = (span + NT - 1) / NT;
    const int k = lo_k + tid * step;
    const bool ok = k < hi_k && (int)lpos[k] < (int)rrev[k];
    const unsigned long long bal = __ballot(ok);
    if ((tid & 63) == 0) S.bc[tid >> 6] = __popcll(bal);
    __syncthreads();
    int good = 0;                                             // probes are monotone: the first `good` probes hold
    for (int w = 0; w < NW; w++) good += S.bc[w];
    __syncthreads();
    if (good == 0) { hi_k = lo_k; break; }
    const int last_good = lo_k + (good - 1) * step;
    lo_k = last_good + 1;
    hi_k = min(hi_k, last_good + step);
  }
  const int m = lo_k;
  for (int k = tid; k < m; k += NT) {
    const int i = (int)lpos[k], j = (int)rrev[k];
    const E t = a[i];
    a[i] = a[j];
    a[j] = t;
  }
  int ret;
  if (MODE == 0) {
    const int Lm = m < cntL ? (int)lpos[m] : CV_NOPOS;
    const int Rm1 = m > 0 ? (int)rrev[m - 1] : CV_NOPOS;
    ret = min(Lm, Rm1);
  } else {
    ret = lo + cntR;
  }
  __syncthreads();   // swaps visible, lists free
  return ret;
}

// ---- libstdc++ heap primitives on an LDS array (one thread): __adjust_heap (with its __push_heap tail), __make_heap
template <class E>
__device__ __forceinline__ void cv_adjust_heap(E* hp, int hole, int len, E value) {
  const int top = hole;
  int child = hole;
  while (child < (len - 1) / 2) {
    child = 2 * (child + 1);
    if (cv_gt(hp[child], hp[child - 1])) child--;
    hp[hole] = hp[child];
    hole = child;
  }
  if ((len & 1) == 0 && child == (len - 2) / 2) {
    child = 2 * (child + 1);
    hp[hole] = hp[child - 1];
    hole = child - 1;
  }
  int parent = (hole - 1) / 2;
  while (hole > top && cv_gt(hp[parent], value)) {
    hp[hole] = hp[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  hp[hole] = value;
}

// std::__heap_select(a + first, a + middle, a + last, greater-by-key), introselect's fall-back when its depth limit is
// reached: the heap [first, middle) lives in LDS while the tail is scanned; the scan is the workgroup's (256 elements per
// step, the next element that beats the heap's top found by ballot), the heap operations are one thread's.
template <class EP>
__device__ __forceinline__ void cv_heap_select(EP a, int first, int middle, int last, typename std::remove_pointer<EP>::type* hp, CvLds& S) {
  typedef typename std::remove_pointer<EP>::type E;
  const int tid = threadIdx.x, len = middle - first, NT = (int)blockDim.x, NW = NT >> 6;
  for (int i = tid; i < len; i += NT) hp[i] = a[first + i];
  __syncthreads();
  if (tid == 0 && len >= 2) {
    int parent = (len - 2) / 2;
    for (;;) {
      const E value = hp[parent];
      cv_adjust_heap(hp, parent, len, value);
      if (parent == 0) break;
      parent--;
    }
  }
  __syncthreads();
  for (int base = middle; base < last; base += NT) {
    const int idx = base + tid;
    const E mine = idx < last ? a[idx] : (E)0;
    int done = base;   // elements of this chunk below `done` have been handled
    for (;;) {
      const E top = hp[0];
      const bool hit = idx < last && idx >= done && cv_gt(mine, top);
      const unsigned long long bal = __ballot(hit);
      if ((tid & 63) == 0) S.bc[tid >> 6] = bal ? (int)(tid + __ffsll((long long)bal) - 1) : 1 << 20;
      __syncthreads();
      int j = 1 << 20;                                                   // thread index of the first hit
      for (int w = 0; w < NW; w++) j = min(j, S.bc[w]);
      __syncthreads();
      if (j >= NT) break;
      if (tid == j) {
        // __pop_heap(first, middle, result = a + idx)
        a[idx] = top;
        cv_adjust_heap(hp, 0, len, mine);
      }
      done = base + j + 1;
      __syncthreads();
    }
  }
  for (int i = tid; i < len; i += NT) a[first + i] = hp[i];
  __syncthreads();
}

// a range that fits the LDS block is worked on in LDS: a round then costs LDS latencies instead of a chain of dependent
// global accesses (pivot, cut, lists), which is what the small pyramid levels and the last rounds of the large ones consist
// of.  The block serves the two retainBest stages one after the other, so its range is counted in bytes: CV_CAP32 32-bit
// elements (first stage) or CV_CAP64 64-bit ones (second stage).  A stopper list can take as many entries as the range has
// elements: with every key equal to the pivot each element is a left and a right stopper, and cv_partition stores up to
// min(cntL, cntR) + 1 of them before it knows how many pair.  2048 / 1024 elements: 16 KB + the heap, eight workgroups per CU
// (measured against 2048 / 2048 at six, 2048 / 1024 at seven and 4096 / 2048 at four: profiles/select_place_ab.txt).
#define CV_CAP32 2048
#define CV_CAP64 1024
#define CV_WAVES_PER_EU 8
#define CV_SMALL_BYTES (CV_CAP32 * 4 > CV_CAP64 * 8 ? CV_CAP32 * 4 : CV_CAP64 * 8)
#define CV_LIST_CAP (CV_CAP32 > CV_CAP64 ? CV_CAP32 : CV_CAP64)
static_assert(CV_LIST_CAP <= 65536, "16-bit positions");
struct CvSmall {
  unsigned long long a[CV_SMALL_BYTES / 8];
  uint16_t l[CV_LIST_CAP], r[CV_LIST_CAP];
};
template <class E>
__device__ __forceinline__ constexpr int cv_small_cap() { return sizeof(E) == 4 ? CV_CAP32 : CV_CAP64; }

// libstdc++ __introselect on a[first, last) with `depth` rounds left; false = the heap of the depth-limit fall-back does
// not fit the LDS array (cannot happen for nth <= 2 * quota: the launcher sizes it so)
template <class EP, class LP>
__device__ __forceinline__ bool cv_introselect_loop(EP a, int first, int nth, int last, int depth, LP lpos, LP rpos, CvLds& S,
                                    unsigned long long* hp_raw, int hp_cap, CvSmall* sm) {
  typedef typename std::remove_pointer<EP>::type E;
  E* hp = reinterpret_cast<E*>(hp_raw);
  while (last - first > 3) {
    if constexpr (std::is_same<LP, uint32_t*>::value) if (sm && last - first <= cv_small_cap<E>()) {   // (the LDS instantiation never stages)
      const int len = last - first;
      E* la = reinterpret_cast<E*>(sm->a);
      for (int i = threadIdx.x; i < len; i += (int)blockDim.x) la[i] = a[first + i];
      __syncthreads();
      const bool ok = cv_introselect_loop<E*, uint16_t*>(la, 0, nth - first, len, depth, sm->l, sm->r, S, hp_raw, hp_cap, nullptr);
      for (int i = threadIdx.x; i < len; i += (int)blockDim.x) a[first + i] = la[i];
      __syncthreads();
      return ok;
    }
    if (depth == 0) {
      if (nth + 1 - first > hp_cap) return false;
      cv_heap_select(a, first, nth + 1, last, hp, S);
      if (threadIdx.x == 0) {
        const E t = a[first];
        a[first] = a[nth];
        a[nth] = t;
      }
      __syncthreads();
      return true;
    }
    --depth;
    // __move_median_to_first(first, first + 1, mid, last - 1), by one thread (having every thread fetch the three candidates
    // and skip the read-back of the pivot measured the same: profiles/r06_select_passes_ab.txt)
    const int ia = first + 1, ib = first + (last - first) / 2, ic = last - 1;
    if (threadIdx.x == 0) {
      const E va = a[ia], vb = a[ib], vc = a[ic];
      int pick;
      if (cv_gt(va, vb)) pick = cv_gt(vb, vc) ? ib : (cv_gt(va, vc) ? ic : ia);
      else pick = cv_gt(va, vc) ? ia : (cv_gt(vb, vc) ? ic : ib);
      const E t = a[first];
      a[first] = a[pick];
      a[pick] = t;
    }
    __syncthreads();
    const uint32_t p = cv_key(a[first]);
    const int cut = cv_partition<0>(a, first + 1, last, p, lpos, rpos, S);
    if (cut <= nth) first = cut; else last = cut;
  }
  if (threadIdx.x == 0) {
    // __insertion_sort(first, last)
    for (int i = first + 1; i < last; i++) {
      const E val = a[i];
      if (cv_gt(val, a[first])) {
        for (int j = i; j > first; j--) a[j] = a[j - 1];
        a[first] = val;
      } else {
        int j = i;
        while (cv_gt(val, a[j - 1])) { a[j] = a[j - 1]; --j; }
        a[j] = val;
      }
    }
  }
  __syncthreads();
  return true;
}

// KeyPointsFilter::retainBest on a[0, n): std::nth_element(a, a + npoints, a + n), then std::partition of the tail by
// "response >= a[npoints - 1].response".  Returns the new size, -1 when the fall-back heap does not fit.
template <class E>
__device__ __forceinline__ int cv_retain_best(E* a, int n, int npoints, uint32_t* lpos, uint32_t* rpos, CvLds& S,
                              unsigned long long* hp, int hp_cap, CvSmall* sm) {
  if (npoints < 0 || n <= npoints) return n;
  if (npoints == 0) return 0;
  const int depth = 2 * (31 - __clz(n));
  if (n <= cv_small_cap<E>()) {              // everything in LDS, the survivors copied back
    E* la = reinterpret_cast<E*>(sm->a);
    for (int i = threadIdx.x; i < n; i += (int)blockDim.x) la[i] = a[i];
    __syncthreads();
    if (!cv_introselect_loop<E*, uint16_t*>(la, 0, npoints, n, depth, sm->l, sm->r, S, hp, hp_cap, nullptr)) return -1;
    const uint32_t amb = cv_key(la[npoints - 1]);
    const int k = cv_partition<1>(la, npoints, n, amb, sm->l, sm->r, S);
    for (int i = threadIdx.x; i < k; i += (int)blockDim.x) a[i] = la[i];
    __syncthreads();
    return k;
  }
  if (!cv_introselect_loop<E*, uint32_t*>(a, 0, npoints, n, depth, lpos, rpos, S, hp, hp_cap, sm)) return -1;
  const uint32_t amb = cv_key(a[npoints - 1]);
  return cv_partition<1>(a, npoints, n, amb, lpos, rpos, S);
}

// ---- the corners of a level in row-major order (as cv::FAST hands them over).  Every FAST tile left its corners as one
// row-major burst in the level's list, with a descriptor (word 0 = offset of the burst, words 1..7 = corners per tile row, a
// byte each).  The place of a corner is
//     (corners in earlier rows of the level) + (corners of its row in tiles to the left) + (its rank in its tile's row),
// and its rank in its tile's row is (its index in the list) - (offset of the burst) - (corners in earlier rows of the tile).
// The work is split by BAND, one row of FAST tiles (FT_H level rows by tiles_x tiles): with
//     base             = corners in earlier bands of the level                              (k_cv_band_base, a prefix of band totals)
//     E[row][tile col] = corners in earlier rows of the band + corners of the row in tiles to the left
//                        - corners in earlier rows of the tile                              (row = row in the band, 0 .. FT_H - 1)
// the place of candidate i of tile column tx is base + E[row][tx] - D[tx].offset + i.  A band's table is 28 x 32 entries at
// the most and its destination is one contiguous range of the sequence, so a band is a small unit that needs nothing but
// its own tiles_x descriptors and its base: a 720p frame has 105 of them, a launch some hundred thousand.
// The index arithmetic is __host__ __device__ and checked on the host against a sort by (y, x): tools/cv_place_host_check.hip.
#define CVP_MAX_TX 32        // tiles per band: widths below 4096 (evh_create) give at most 32
#define CVP_MAX_BANDS 160    // bands per level: heights below 4096 give at most 145
#define CVP_NT 64            // k_cv_place: one wave per band (2, 4 and 8 bands per workgroup measured the same)
#define CVP_TILE_CHUNKS 16   // chunks of CVP_NT corners per tile: k_fast_main's list of a tile holds 1024
#define CVP_EPT 16           // chunks per step: sixteen loads in flight per lane (4: +0.13 ms, 8: +0.06 ms per launch of 2048 720p frames)

__host__ __device__ __forceinline__ int cvp_word_sum(uint32_t w) {   // the four bytes of a descriptor word added up
  const uint32_t p = (w & 0x00FF00FFu) + ((w >> 8) & 0x00FF00FFu);
  return (int)((p & 0xFFFFu) + (p >> 16));
}
// corners of tile row r (0 .. FT_H - 1) of the tile whose descriptor is d[0..8)
__host__ __device__ __forceinline__ int cvp_corners(const uint32_t* d, int r) { return (int)((d[1 + (r >> 2)] >> (8 * (r & 3))) & 0xFFu); }
__host__ __device__ __forceinline__ int cvp_tile_total(const uint32_t* d) {
  int s = 0;
  for (int w = 1; w < 8; w++) s += cvp_word_sum(d[w]);
  return s;
}
// E[row][tx] from: rows_before = corners in earlier rows of the band, left = corners of the row in tiles to the left,
// tile_before = corners in earlier rows of the tile
__host__ __device__ __forceinline__ int cvp_entry(int rows_before, int left, int tile_before) { return rows_before + left - tile_before; }
// row in band ty of the level that a candidate's y names (clamped: a candidate always lies in the band of its tile)
__host__ __device__ __forceinline__ int cvp_band_row(uint32_t c, int ty) {
  const int r = (int)((c >> 12) & 0xFFFu) - EVH_FAST_OY - ty * FT_H;
  return r < 0 ? 0 : (r > FT_H - 1 ? FT_H - 1 : r);
}
// a burst is taken in chunks of CVP_NT corners: the list entry of chunk q of tile column tx, and the chunk's first corner
__host__ __device__ __forceinline__ uint16_t cvp_chunk(int tx, int q) { return (uint16_t)(tx | (q << 8)); }
__host__ __device__ __forceinline__ int cvp_chunk_first(int w) { return (w >> 8) * CVP_NT; }
// place of candidate i of a tile whose burst starts at off: base = the band's, e = E[row][tx]
__host__ __device__ __forceinline__ int cvp_place(int base, int e, int off, int i) { return base + e - off + i; }

// the level of band b of a frame and b's index inside the level
__device__ __forceinline__ int cvp_level_of_band(const SelCvArgs& B, int& b) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < EVH_NLEVELS; i++)
    if (b >= B.band_start[i]) l = i;
  b -= B.band_start[l];
  return l;
}

// Pre-pass, one workgroup per (level, frame): the level's descriptors are read once, the corners of each band added up and
// their exclusive prefix written to B.band (the band bases), the level's total behind the frame's bands.
__global__ __launch_bounds__(256) void k_cv_band_base(SelCvArgs B) {
  const SelectArgs& A = B.s;
  __shared__ int bs[CVP_MAX_BANDS];
  int l, f;
  xcd_order(l, f);
  if (f >= A.nframes || l >= EVH_NLEVELS) return;
  const int tid = threadIdx.x, NT = (int)blockDim.x;
  const EvhLevel L = A.lv[l];
  const int n = min(A.cand_count[f * EVH_NLEVELS + l], L.cand_cap);
  if (n <= 0 || L.quota <= 0) return;          // no placement, and k_select_cv does not ask for the total
  const int TX = L.tiles_x, TY = min(L.tiles_y, CVP_MAX_BANDS);
  const uint4* td = reinterpret_cast<const uint4*>(B.tdesc + ((int64_t)f * B.total_tiles + L.tile_start) * 8);
  for (int b = tid; b < TY; b += NT) bs[b] = 0;
  __syncthreads();
  for (int t = tid; t < TX * TY; t += NT) {
    const uint4 lo = td[2 * t], hi = td[2 * t + 1];
    const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const int c = cvp_tile_total(d);
    if (c) atomicAdd(&bs[t / TX], c);
  }
  __syncthreads();
  if (tid < 64) {                              // exclusive prefix over the bands, 64 at a step
    int* out = B.band + (int64_t)f * B.band_frame_entries;
    int carry = 0;
    for (int b0 = 0; b0 < TY; b0 += 64) {
      const int b = b0 + tid, v = b < TY ? bs[b] : 0;
      const int incl = wave_scan_incl(v);
      if (b < TY) out[B.band_start[l] + b] = carry + incl - v;
      carry += __builtin_amdgcn_readlane(incl, 63);
    }
    if (tid == 0) out[B.nbands + l] = carry;
  }
}

struct CvpLds {
  int E[FT_H * CVP_MAX_TX];
  uint16_t W[CVP_MAX_TX * CVP_TILE_CHUNKS];
};

// Placement, one wave per band.  Lane tx holds the descriptor of tile column tx in registers; row by row a scan over the
// lanes gives the corners to the left, two running sums the corners in earlier rows of the band and of the tile: E goes to
// LDS with no load behind it.  Then the bursts, 64 corners (a chunk) at a time; offset and corners of a chunk's tile are
// the wave's, read off lane tx; a lane takes one corner of the chunk: one coalesced load, one table entry, one store.
// Candidates whose place or whose index falls outside [0, n) are dropped (never: descriptors and list come from the same tiles).
__global__ __launch_bounds__(CVP_NT) void k_cv_place(SelCvArgs B) {
  const SelectArgs& A = B.s;
  __shared__ CvpLds S;
  static_assert(CVP_NT == 64 && CVP_MAX_TX <= 64, "one wave, a lane per tile column");
  int ty, f;
  xcd_order(ty, f);
  if (f >= A.nframes || ty >= B.nbands) return;
  const int band = ty;
  const int l = cvp_level_of_band(B, ty);
  const int lane = threadIdx.x;
  const EvhLevel L = A.lv[l];
  const int n = min(A.cand_count[f * EVH_NLEVELS + l], L.cand_cap);
  if (n <= 0 || L.quota <= 0 || ty >= CVP_MAX_BANDS) return;
  const int TX = min(L.tiles_x, CVP_MAX_TX);
  const uint4* td = reinterpret_cast<const uint4*>(B.tdesc + ((int64_t)f * B.total_tiles + L.tile_start + ty * L.tiles_x) * 8);
  const int base = B.band[(int64_t)f * B.band_frame_entries + band];
  uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
  if (lane < TX) { lo = td[2 * lane]; hi = td[2 * lane + 1]; }
  const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  int tile_before = 0, rows_before = 0;
#pragma unroll
  for (int r = 0; r < FT_H; r++) {
    const int c = cvp_corners(d, r);            // 0 in the lanes past TX
    const int incl = wave_scan_incl(c);
    if (lane < TX) S.E[r * TX + lane] = cvp_entry(rows_before, incl - c, tile_before);
    rows_before += __builtin_amdgcn_readlane(incl, 63);
    tile_before += c;
  }
  // the band's chunks, tile by tile: lane tx lists those of its tile
  const int nch = min((tile_before + CVP_NT - 1) / CVP_NT, CVP_TILE_CHUNKS);   // 0 in the lanes past TX
  const int incl_ch = wave_scan_incl(nch);
  const int nchunks = __builtin_amdgcn_readlane(incl_ch, 63);
  for (int q = 0; q < nch; q++) S.W[incl_ch - nch + q] = cvp_chunk(lane, q);
  __syncthreads();
  const uint32_t* cand = A.cand + (int64_t)f * A.cand_frame_entries + L.cand_off;
  uint32_t* out = B.seq32 + (int64_t)f * A.cand_frame_entries + L.cand_off;
  // the bursts in chunks of 64 corners, CVP_EPT chunks a step: the loads of a step are issued together (chunk by chunk a wave
  // would wait for memory once per chunk, some twenty times for a level-0 band of a 720p frame)
  for (int k0 = 0; k0 < nchunks; k0 += CVP_EPT) {
    uint32_t c[CVP_EPT];
    int tx[CVP_EPT], off[CVP_EPT], idx[CVP_EPT];
#pragma unroll
    for (int s = 0; s < CVP_EPT; s++) {
      const int w = __builtin_amdgcn_readfirstlane((int)S.W[min(k0 + s, nchunks - 1)]);
      tx[s] = w & 0xFF;
      off[s] = __builtin_amdgcn_readlane((int)d[0], tx[s]);
      const int j = cvp_chunk_first(w) + lane, cnt = __builtin_amdgcn_readlane(tile_before, tx[s]);
      idx[s] = (int)((uint32_t)off[s] + (uint32_t)j);
      if (k0 + s >= nchunks || j >= cnt || (unsigned)idx[s] >= (unsigned)n) idx[s] = -1;
      c[s] = cand[max(idx[s], 0)];
    }
#pragma unroll
    for (int s = 0; s < CVP_EPT; s++) {
      if (idx[s] < 0) continue;
      const int e = S.E[cvp_band_row(c[s], ty) * TX + tx[s]];
      const int pos = cvp_place(base, e, off[s], idx[s]);
      if ((unsigned)pos < (unsigned)n) out[pos] = c[s];
    }
  }
}

// One workgroup of 256 threads per (level, frame), started when the row-major sequence of every level lies in seq32.
// 63 VGPRs, no scratch, 16.2 KB static LDS + the heap: eight workgroups per CU.  The bounds ask for that occupancy outright:
// under looser ones the compiler spends 128 VGPRs, and every device function has to be inlined (left as a call, its
// callee-saved registers go to scratch).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CV_WAVES_PER_EU))) void k_select_cv(SelCvArgs B) {
  const SelectArgs& A = B.s;
  __shared__ CvLds S;
  __shared__ CvSmall SM;
  extern __shared__ unsigned long long cv_heap[];   // 2 * quota(level 0) + 2 entries
  int l, f;
  xcd_order(l, f);
  if (f >= A.nframes || l >= EVH_NLEVELS) return;
  const int tid = threadIdx.x, NT = (int)blockDim.x;
  const EvhLevel L = A.lv[l];
  const int n_raw = A.cand_count[f * EVH_NLEVELS + l];
  bool overflow = n_raw > L.cand_cap;
  const int n = min(n_raw, L.cand_cap);
  const int q = L.quota;
  unsigned long long* a = B.seq + (int64_t)f * A.cand_frame_entries + L.cand_off;
  uint32_t* a32 = B.seq32 + (int64_t)f * A.cand_frame_entries + L.cand_off;
  uint32_t* lpos = B.lpos + (int64_t)f * A.cand_frame_entries + L.cand_off;
  uint32_t* rpos = B.rpos + (int64_t)f * A.cand_frame_entries + L.cand_off;
  int k2 = 0;
  bool unsupported = false;
  if (n > 0 && q > 0) {
    // the corners the level's descriptors count (k_cv_band_base)
    if (B.band[(int64_t)f * B.band_frame_entries + B.nbands + l] != n) overflow = true;    // cannot happen: the descriptors and the list come from the same tiles
    if (B.phase_limit == 1) { if (tid == 0) A.lvl_count[f * EVH_NLEVELS + l] = 0; return; }   // (no key points: nothing downstream reads what was not written)
    // ---- retainBest(2 * quota) by FAST score
    int k1 = cv_retain_best(a32, n, 2 * q, lpos, rpos, S, cv_heap, B.heap_cap, &SM);
    if (k1 < 0) { unsupported = true; k1 = 0; }
    if (B.phase_limit == 2) { if (tid == 0) A.lvl_count[f * EVH_NLEVELS + l] = 0; return; }   // (no key points: nothing downstream reads what was not written)
    // ---- Harris response of the survivors, in place
    const uint8_t* img = A.pyr + (int64_t)f * A.pyr_frame_bytes + L.off;
    for (int j = tid; j < k1; j += NT) {
      const uint32_t c = a32[j];
      const float r = harris_response(img, L.stride, cand_x(c), cand_y(c));
      a[j] = ((unsigned long long)f32_order_key(r) << 32) | c;
    }
    __syncthreads();
    // ---- retainBest(quota) by Harris response
    k2 = cv_retain_best(a, k1, q, lpos, rpos, S, cv_heap, B.heap_cap, &SM);
    if (k2 < 0) { unsupported = true; k2 = 0; }
    if (k2 > A.kcap) { overflow = true; k2 = A.kcap; }
    for (int j = tid; j < k2; j += NT) {
      const unsigned long long e = a[j];
      const int64_t o = ((int64_t)f * EVH_NLEVELS + l) * A.kcap + j;
      A.tmp_meta[o] = ((uint32_t)l << 24) | ((uint32_t)e & 0xFFFFFFu);
      A.tmp_resp[o] = f32_from_order_key((uint32_t)(e >> 32));
    }
  }
  if (tid == 0) {
    A.lvl_count[f * EVH_NLEVELS + l] = k2;
    if (overflow) atomicOr(&A.frame_flags[f], 1);
    if (unsupported) atomicOr(&A.frame_flags[f], 2);
  }
}
}  // namespace
