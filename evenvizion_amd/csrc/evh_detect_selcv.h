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
//   * the row-major sequence comes from one pass over the level's list: a candidate's x and y name its tile and row, small
//     tables built from the FAST tile descriptors turn them into its place (cv_build_tables / cv_place).
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
  uint32_t* mask;            // [nframes][2 * mask_frame_words] scratch of the row-major tables that do not fit LDS (E | RB)
  int64_t mask_frame_words;
  int mask_off[EVH_NLEVELS];
  const uint32_t* tdesc;     // [nframes][total_tiles][8] tile burst descriptors written by k_fast
  int total_tiles;
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

// a range of at most CV_SMALL elements is worked on in LDS: a round then costs LDS latencies instead of a chain of
// dependent global accesses (pivot, cut, lists), which is what the small pyramid levels and the last rounds of the large
// ones consist of
#define CV_SMALL 2048
struct CvSmall {
  unsigned long long a[CV_SMALL];
  uint16_t l[CV_SMALL], r[CV_SMALL];
};
#define CV_TAB_BYTES ((int)sizeof(CvSmall))   // what the row-major tables of a level may take of it

// libstdc++ __introselect on a[first, last) with `depth` rounds left; false = the heap of the depth-limit fall-back does
// not fit the LDS array (cannot happen for nth <= 2 * quota: the launcher sizes it so)
template <class EP, class LP>
__device__ __forceinline__ bool cv_introselect_loop(EP a, int first, int nth, int last, int depth, LP lpos, LP rpos, CvLds& S,
                                    unsigned long long* hp_raw, int hp_cap, CvSmall* sm) {
  typedef typename std::remove_pointer<EP>::type E;
  E* hp = reinterpret_cast<E*>(hp_raw);
  while (last - first > 3) {
    if constexpr (std::is_same<LP, uint32_t*>::value) if (sm && last - first <= CV_SMALL) {   // (the LDS instantiation never stages)
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
// staged: the sequence already lies in sm->a and not in a (n > npoints and n <= CV_SMALL then; the survivors go to a)
template <class E>
__device__ __forceinline__ int cv_retain_best(E* a, int n, int npoints, uint32_t* lpos, uint32_t* rpos, CvLds& S,
                              unsigned long long* hp, int hp_cap, CvSmall* sm, bool staged = false) {
  if (npoints < 0 || n <= npoints) return n;
  if (npoints == 0) return 0;
  const int depth = 2 * (31 - __clz(n));
  if (n <= CV_SMALL) {                       // everything in LDS, the survivors copied back
    E* la = reinterpret_cast<E*>(sm->a);
    if (!staged) {
      for (int i = threadIdx.x; i < n; i += (int)blockDim.x) la[i] = a[i];
      __syncthreads();
    }
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
// row-major burst in the level's list, with a descriptor (offset of the burst, corners per tile row).  The place of a corner is
//     (corners in earlier rows of the level) + (corners of its row in tiles to the left) + (its rank in its tile's row),
// and its rank in its tile's row is (its index in the list) - (offset of the burst) - (corners in earlier rows of the tile).
// A candidate word carries x and y, hence its tile and row, so with
//     RB[row]          = corners in earlier rows of the level                               (row = tile row * FT_H + row in the tile)
//     E[row][tile col] = corners of the row in tiles to the left - corners in earlier rows of the tile   (16 bits: |E| < 4096)
// the place of candidate i is RB[row] + E[row][tx] - D[tile].offset + i: one pass over the list with independent, coalesced
// loads, three table reads each.  D, RB and E lie in LDS where they fit (CvSmall is idle until the sequence exists), else in
// the per-frame global scratch; the pass is the same.  D: descriptors (8 words per tile).  Returns the corners the descriptors count.
template <class TD, class TR, class TE>
__device__ __forceinline__ int cv_build_tables(TD D, TR RB, TE E, int TX, int TY, CvLds& S) {
  const int tid = threadIdx.x, NT = (int)blockDim.x, NR = TY * FT_H;
  auto corners = [&](int t, int r) { return (int)((D[t * 8 + 1 + (r >> 2)] >> (8 * (r & 3))) & 0xFFu); };
  // rows of the level, `per` consecutive ones per thread: E = corners to the left in the row, RB by a scan of the row totals
  const int per = (NR + NT - 1) / NT, r0 = min(NR, tid * per), r1 = min(NR, r0 + per);
  int sum = 0;
  for (int row = r0; row < r1; row++) {
    const int ty = row / FT_H, r = row - ty * FT_H;
    int in = 0;
    for (int tx = 0; tx < TX; tx++) { E[row * TX + tx] = (int16_t)in; in += corners(ty * TX + tx, r); }
    RB[row] = in;
    sum += in;
  }
  int ex, d0, tot, d1;
  cv_scan2(S, sum, 0, ex, d0, tot, d1);
  for (int row = r0; row < r1; row++) { const int c = RB[row]; RB[row] = ex; ex += c; }
  __syncthreads();
  // tiles: take the corners in earlier rows of the tile off E
  for (int t = tid; t < TX * TY; t += NT) {
    const int ty = t / TX, tx = t - ty * TX;
    int before = 0;
#pragma unroll 4
    for (int r = 0; r < FT_H; r++) {
      E[(ty * FT_H + r) * TX + tx] -= (int16_t)before;
      before += corners(t, r);
    }
  }
  __syncthreads();
  return tot;
}

// cand[0, n) -> out[place]; candidates the tables cannot place (never: descriptors and list come from the same tiles) are dropped
template <class TD, class TR, class TE, class TO>
__device__ __forceinline__ void cv_place(const uint32_t* cand, int n, TD D, TR RB, TE E, int TX, int TY, TO out) {
#pragma unroll 4
  for (int i = threadIdx.x; i < n; i += (int)blockDim.x) {
    const uint32_t c = cand[i];
    const int tx = min(max(cand_x(c) - EVH_FAST_OX, 0) / FT_W, TX - 1);
    const int row = min(max(cand_y(c) - EVH_FAST_OY, 0), TY * FT_H - 1);
    const int pos = RB[row] + (int)E[row * TX + tx] - (int)D[((row / FT_H) * TX + tx) * 8] + i;
    if ((unsigned)pos < (unsigned)n) out[pos] = c;
  }
}

// One workgroup of 256 threads per (level, frame).  65 VGPRs, no scratch, 24.2 KB static LDS + the heap: six workgroups per CU.
// The bounds ask for that occupancy outright; under looser ones the compiler spends 128 VGPRs, and every device function has to
// be inlined (left as a call, its callee-saved registers go to scratch).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void k_select_cv(SelCvArgs B) {
  const SelectArgs& A = B.s;
  __shared__ CvLds S;
  __shared__ CvSmall SM;
  extern __shared__ unsigned long long cv_heap[];   // 2 * quota(level 0) + 2 entries
  int l, f;
  xcd_order(l, f);
  if (f >= A.nframes || l >= EVH_NLEVELS) return;
  const int tid = threadIdx.x, NT = (int)blockDim.x;
  const EvhLevel L = A.lv[l];
  const uint32_t* cand = A.cand + (int64_t)f * A.cand_frame_entries + L.cand_off;
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
    // ---- the row-major sequence (cv_build_tables).  Where the tables lie:
    //   * in CvSmall when D + RB + E fit its CV_TAB_BYTES (720p level 0, 10 x 24 tiles: 23.8 KB; 1080p level 0 and 4K levels
    //     0..2 do not fit) -- and behind the first CV_SMALL words of it when the sequence itself fits those and retainBest is
    //     going to work on it in LDS: the pass then writes it there, with no global copy in between;
    //   * else in the frame's global scratch (B.mask: E in the level's slice of the first half, RB of the second), D read in place.
    const int TX = L.tiles_x, TY = L.tiles_y, NR = TY * FT_H;
    const int tab_bytes = TX * TY * 32 + NR * 4 + NR * TX * 2;
    const bool staged = n > 2 * q && n <= CV_SMALL && tab_bytes <= CV_TAB_BYTES - CV_SMALL * 4;
    const uint32_t* td = B.tdesc + ((int64_t)f * B.total_tiles + L.tile_start) * 8;
    int tot;
    if (staged || tab_bytes <= CV_TAB_BYTES) {
      uint32_t* D = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(&SM) + (staged ? CV_SMALL * 4 : 0));
      int* RB = reinterpret_cast<int*>(D + TX * TY * 8);
      int16_t* E = reinterpret_cast<int16_t*>(RB + NR);
      for (int i = tid; i < TX * TY * 8; i += NT) D[i] = td[i];
      __syncthreads();
      tot = cv_build_tables(D, RB, E, TX, TY, S);
      if (staged) cv_place(cand, n, D, RB, E, TX, TY, reinterpret_cast<uint32_t*>(SM.a));
      else cv_place(cand, n, D, RB, E, TX, TY, a32);
    } else {
      uint32_t* P = B.mask + (int64_t)f * 2 * B.mask_frame_words + B.mask_off[l];
      int* RB = reinterpret_cast<int*>(P + B.mask_frame_words);
      int16_t* E = reinterpret_cast<int16_t*>(P);
      tot = cv_build_tables(td, RB, E, TX, TY, S);
      cv_place(cand, n, td, RB, E, TX, TY, a32);
    }
    if (tot != n) overflow = true;    // cannot happen: the descriptors and the list come from the same tiles
    __syncthreads();
    if (B.phase_limit == 1) { if (tid == 0) A.lvl_count[f * EVH_NLEVELS + l] = 0; return; }   // (no key points: nothing downstream reads what was not written)
    // ---- retainBest(2 * quota) by FAST score
    int k1 = cv_retain_best(a32, n, 2 * q, lpos, rpos, S, cv_heap, B.heap_cap, &SM, staged);
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
