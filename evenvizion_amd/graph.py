"""Global alignment: every superposed matrix of a video adjusted at once, so that the frames agree wherever they see the same ground.

The dictionary's S_k is a product of k pair matrices, and its error grows along the chain.  Here the match rows of many frame pairs
("edges": every consecutive pair, and pairs of frames far apart in time whose footprints on the plane overlap -- a loop) enter ONE
least-squares problem over all S_k: a row (a in frame i, b in frame j) asks that S_i.a and S_j.b be the same plane point.  The normal
equations of that problem are summed on the device (evh_graph_normal, include/evhip.h states the arithmetic), 154 doubles per edge;
the solve is dense float64 on the host.

    graph_normal(ctx, S, edges, rows, counts, ...)      the device call -> (sums, info) device tensors
    assemble(sums, edges, nframes)                      -> the symmetric matrix of 8*nframes and the gradient
    BASIS                                               the motion models, as 8 x d matrices the blocks are projected through
    solve_graph(S, evaluate, model, iters, fixed)       damped Gauss-Newton over the corrections D_k, S'_k = D_k . S_k
    loop_candidates(superposition, resize_info, ...)    which pairs of frames to match
    align_superposition / aligned_homography_dict       the drivers: read the video, match the pairs, solve, write the dictionary
"""
import numpy as np

from . import runtime
from .frames import DeviceLadder, FrameReader, check_ingest, entry_matrix

NSUMS = 154
MODELS = ("translation", "similarity", "affine", "homography")
NODE_BYTES_BUDGET = 1 << 30          # the node frames kept on the device at the working size
MAX_NODES = 512                      # the host solve is dense: 512 nodes are a matrix of 4096 x 4096 doubles, 128 MiB
PAIRS_PER_CALL = 64                  # candidate pairs matched per pair_homography_batch call


def _basis():
    e = np.eye(8)
    return {"translation": e[:, [2, 5]],
            "similarity": np.stack([e[:, 0] + e[:, 4], e[:, 3] - e[:, 1], e[:, 2], e[:, 5]], axis=1),     # a, b, tx, ty
            "affine": e[:, :6],
            "homography": e}


BASIS = _basis()


# ---- the device call and what becomes of its sums ---------------------------------------------------------------------------------------
def graph_normal(ctx, S, edges, rows, counts, status=None, H_edge=None, inlier_thr=3.0, huber_delta=0.0):
    """evh_graph_normal through Context.graph_normal.  S f64[nframes,3,3], edges [nedges,2] = (i, j) and H_edge f64[nedges,3,3] or
    None may be arrays or tensors (they are taken to the device); rows f32[nedges,cap,4], counts and status are tensors as
    Context.batch_static_rows returns them, or arrays.  -> (sums f64[nedges,154], info i32[nedges,4]) device tensors.  torch's
    current stream is ordered behind the launch before this returns: the uploaded copies may go back to the allocator, and the
    results may be used by torch operations, without a further wait."""
    import torch
    dev = torch.device("cuda", ctx.device)

    def to(t, dtype):
        if t is None:
            return None
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.ascontiguousarray(t))
        return t.to(device=dev, dtype=dtype).contiguous()
    S, H_edge = to(S, torch.float64), to(H_edge, torch.float64)
    out = ctx.graph_normal(S.reshape(-1), to(edges, torch.int32).reshape(-1, 2), to(rows, torch.float32), to(counts, torch.int32),
                           to(status, torch.int32), None if H_edge is None else H_edge.reshape(-1), inlier_thr, huber_delta)
    ctx.order_torch_after()
    return out


def _triu_to_full(tri):
    A = np.zeros((8, 8))
    A[np.triu_indices(8)] = tri
    return A + np.triu(A, 1).T


def assemble(sums, edges, nframes):
    """sums f64[nedges,154] (host), edges [nedges,2] -> (A f64[8 nframes, 8 nframes] symmetric, g f64[8 nframes]): edge (i, j)
    adds A_ii and A_jj to the diagonal blocks, A_ij and its transpose to the blocks (i, j) and (j, i), g_i and g_j to the gradient.
    An edge whose indices the device flags (outside [0, nframes), or i == j) adds nothing."""
    sums, edges = np.asarray(sums, np.float64).reshape(-1, NSUMS), np.asarray(edges).reshape(-1, 2)
    A, g = np.zeros((8 * nframes, 8 * nframes)), np.zeros(8 * nframes)
    for s, (i, j) in zip(sums, edges):
        if not (0 <= i < nframes and 0 <= j < nframes) or i == j:
            continue
        si, sj = slice(8 * i, 8 * i + 8), slice(8 * j, 8 * j + 8)
        A[si, si] += _triu_to_full(s[0:36])
        A[sj, sj] += _triu_to_full(s[36:72])
        Aij = s[72:136].reshape(8, 8)
        A[si, sj] += Aij
        A[sj, si] += Aij.T
        g[si] += s[136:144]
        g[sj] += s[144:152]
    return A, g


def evaluator(normal, edges):
    """normal(S f64[n,3,3]) -> (sums, info), arrays or device tensors (the device call, or the restatement)  ->  evaluate(S) ->
    (A, g, cost) as solve_graph takes it: the assembled system and the cost, the sum of rho over all edges."""
    edges = np.asarray(edges).reshape(-1, 2)

    def evaluate(S):
        sums = normal(S)[0]
        sums = sums.cpu().numpy() if hasattr(sums, "cpu") else np.asarray(sums)
        A, g = assemble(sums, edges, len(S))
        return A, g, float(sums[:, 152].sum())
    return evaluate


def _delta(x):
    D = np.eye(3)
    D.reshape(-1)[:8] += x
    return D


def solve_graph(S, evaluate, model="homography", iters=10, fixed=0, N=None):
    """Damped Gauss-Newton (Levenberg-Marquardt on the diagonal) over all frames at once, float64 on the host.  S: f64[n,3,3];
    evaluate(S) -> (A, g, cost) at those matrices (evaluator above); model: a key of BASIS, the blocks are projected through it;
    frame `fixed` is held.  Each of the `iters` steps solves (A + lambda diag A) x = -g over the free frames' parameters, forms
    S_k <- (I + Delta_k) . S_k / [2][2] and evaluates there; it is accepted only if the cost falls (lambda / 10), else dropped
    (lambda * 10): the cost never rises.  A cost or gradient that is not finite at the start is a ValueError, at a trial step the
    step is dropped.  N: a 3 x 3 matrix the plane is normalised by -- evaluate sees N . S_k, and the result
    comes back through N^-1.  -> (S' f64[n,3,3], {"cost_before", "cost_after", "steps", "accepted", "evaluations"})."""
    if model not in BASIS:
        raise ValueError("model must be one of %s" % ", ".join(MODELS))
    S = np.array(S, np.float64).reshape(-1, 3, 3)
    n = len(S)
    if not 0 <= int(fixed) < n:
        raise ValueError("fixed must name one of the %d frames" % n)
    if isinstance(iters, bool) or int(iters) != iters or int(iters) < 0:
        raise ValueError("iters must be an integer of at least 0")
    N = np.eye(3) if N is None else np.asarray(N, np.float64).reshape(3, 3)
    cur = np.stack([np.dot(N, m) for m in S])
    B = BASIS[model]
    d = B.shape[1]
    free = [k for k in range(n) if k != int(fixed)]
    m = len(free)

    def reduced(A, g):
        """the free frames' blocks, each projected through the model: B^T A_kl B and B^T g_k"""
        A4 = A.reshape(n, 8, n, 8)[free][:, :, free]
        return np.einsum("ar,iajb,bs->irjs", B, A4, B).reshape(m * d, m * d), np.dot(g.reshape(n, 8)[free], B).reshape(-1)
    A, g, cost = evaluate(cur)
    if not np.isfinite(cost) or not np.isfinite(g).all():
        raise ValueError("the cost or the gradient at the matrices handed in is not finite: some edge's sums are not (a matrix that "
                         "sends points to infinity?)")
    report = {"steps": 0, "accepted": 0, "evaluations": 1, "cost_before": cost, "cost_after": cost}
    if int(iters) == 0 or not free:
        return S, report
    lam = 1e-4
    for _ in range(int(iters)):
        if not cost > 0:
            break
        Ar, gr = reduced(A, g)
        diag = np.diag(Ar).copy()
        diag[diag <= 0] = 1.0
        report["steps"] += 1
        try:
            x = np.linalg.solve(Ar + lam * np.diag(diag), -gr)
        except np.linalg.LinAlgError:
            lam *= 10.0
            continue
        full = np.dot(x.reshape(m, d), B.T)
        trial = cur.copy()
        for c, k in enumerate(free):
            T = np.dot(_delta(full[c]), cur[k])
            trial[k] = T / T[2, 2]
        if not np.isfinite(trial).all():
            lam *= 10.0
            continue
        A1, g1, cost1 = evaluate(trial)
        report["evaluations"] += 1
        if cost1 < cost and np.isfinite(g1).all():              # a cost that is not finite compares false: the step is dropped
            cur, A, g, cost, lam = trial, A1, g1, cost1, max(lam / 10.0, 1e-12)
            report["accepted"] += 1
        else:
            lam *= 10.0
    report["cost_after"] = cost
    Ninv = np.linalg.inv(N)
    out = np.stack([np.dot(Ninv, m) for m in cur])
    return out / out[:, 2:3, 2:3], report


# ---- the plane, the footprints and the pairs worth matching -------------------------------------------------------------------------------
def plane_normalisation(superposition, resize_info):
    """-> (N f64[3,3], scale): the similarity that centres stabilization.fixed_plane_bounds of the dictionary and scales its
    longer side to 2, so that plane coordinates are about unit size; a length of the plane in pixels times `scale` is its
    length in the normalised plane (huber_delta goes through that)."""
    from .stabilization import fixed_plane_bounds
    ox, oy, dw, dh = fixed_plane_bounds(superposition, resize_info, max_pixels=1 << 62)
    s = 2.0 / max(dw, dh, 1)
    return np.array([[s, 0, -s * (ox + dw / 2.0)], [0, s, -s * (oy + dh / 2.0)], [0, 0, 1]], np.float64), s


def _footprint(S, w, h):
    """the frame's corners on the plane, in order around the frame, f64[4,2]; None when the matrix is missing or its horizon crosses the frame"""
    if not np.isfinite(S).all():
        return None
    c = np.array([[0, 0, 1], [w, 0, 1], [w, h, 1], [0, h, 1]], np.float64).T
    p = np.dot(S, c)
    if not (np.all(p[2] > 0) or np.all(p[2] < 0)):
        return None
    q = (p[:2] / p[2]).T
    return q if np.isfinite(q).all() else None


def _area(poly):
    x, y = poly[:, 0], poly[:, 1]
    return 0.5 * float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def _clip(subject, clipper):
    """Sutherland-Hodgman: the convex polygon `subject` inside the convex polygon `clipper` (both counter-clockwise) -> f64[m,2]"""
    out = [tuple(p) for p in subject]
    for k in range(len(clipper)):
        a, b = clipper[k], clipper[(k + 1) % len(clipper)]
        side = lambda p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
        inp, out = out, []
        for m in range(len(inp)):
            p, q = inp[m], inp[(m + 1) % len(inp)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        if not out:
            break
    return np.array(out, np.float64).reshape(-1, 2)


def footprint_overlap(Si, Sj, w, h):
    """The part of frame i's footprint on the plane that frame j's covers, 0..1 (0 where either has none)."""
    a, b = _footprint(np.asarray(Si, np.float64).reshape(3, 3), w, h), _footprint(np.asarray(Sj, np.float64).reshape(3, 3), w, h)
    if a is None or b is None:
        return 0.0
    a = a if _area(a) > 0 else a[::-1]
    b = b if _area(b) > 0 else b[::-1]
    whole = _area(a)
    if not whole > 0:
        return 0.0
    both = _clip(a, b)
    return min(1.0, max(0.0, _area(both) / whole)) if len(both) >= 3 else 0.0


def _whole(value, lo, name):
    if isinstance(value, bool) or int(value) != value or int(value) < lo:
        raise ValueError("%s must be an integer of at least %d" % (name, lo))
    return int(value)


def loop_candidates(superposition, resize_info, min_gap=8, min_overlap=0.3, max_partners=4):
    """Which pairs of frames to match, from the dictionary alone (host only).  Frames are numbered 0.. in the dictionary's order.
    -> ([(i, j)], {i: [j, ...]}): every consecutive pair (k, k - 1) first, in order; then, for frame i, the frames j < i - min_gap
    whose footprint on the plane covers at least `min_overlap` of frame i's: the best overlap first (ties: the earlier frame), no
    two partners of a frame within min_gap of each other, at most max_partners per frame.  The second value holds the loop
    partners per frame."""
    min_gap, max_partners = _whole(min_gap, 1, "min_gap"), _whole(max_partners, 0, "max_partners")
    if isinstance(min_overlap, bool) or not 0 < float(min_overlap) <= 1:
        raise ValueError("min_overlap must lie in (0, 1]")
    w, h = float(resize_info["w"]), float(resize_info["h"])
    mats = [entry_matrix(v) for k, v in superposition.items() if k != "resize_info"]
    edges = [(k, k - 1) for k in range(1, len(mats))]
    loops = {}
    for i in range(len(mats)):
        scored = []
        for j in range(0, i - min_gap):
            o = footprint_overlap(mats[i], mats[j], w, h)
            if o >= float(min_overlap):
                scored.append((-o, j))
        taken = []
        for _, j in sorted(scored):
            if len(taken) >= max_partners:
                break
            if all(abs(j - t) >= min_gap for t in taken):
                taken.append(j)
        if taken:
            loops[i] = taken
            edges.extend((i, j) for j in taken)
    return edges, loops


def keep_edges(status, info, min_inliers):
    """status i[nedges] (the pairs' final status), info i[nedges,4] (evh_graph_normal's rows) -> bool[nedges]: the status is
    PAIR_OK, the edge carries no flag and at least min_inliers of its rows passed the gate."""
    status, info = np.asarray(status).reshape(-1), np.asarray(info).reshape(-1, 4)
    return (status == 0) & (info[:, 3] == 0) & (info[:, 0] >= int(min_inliers))


def check_connected(edges, nnodes, fixed=0):
    """ValueError unless the edges connect every one of the nnodes frames to frame `fixed`: a frame no kept edge reaches has no
    equation, and the joint problem no solution."""
    parent = list(range(nnodes))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j in np.asarray(edges).reshape(-1, 2):
        parent[find(int(i))] = find(int(j))
    lost = [k for k in range(nnodes) if find(k) != find(int(fixed))]
    if lost:
        raise ValueError("the kept edges do not connect %d of the %d node frames to frame %d (the first: node %d): matching failed "
                         "there -- lower min_inliers or choose another stride" % (len(lost), nnodes, int(fixed), lost[0]))


def spread_corrections(S, nodes, S_nodes):
    """S: every frame's matrix f64[n,3,3]; nodes: the indices of the node frames, ascending, nodes[0] == 0; S_nodes: their aligned
    matrices.  A frame between two nodes gets the correction D = S'_node . S_node^-1 of the node before it: S'_k = D . S_k / [2][2]
    (a frame whose matrix is not finite stays as it is)."""
    out = np.array(S, np.float64).reshape(-1, 3, 3).copy()
    for pos, k0 in enumerate(nodes):
        k1 = nodes[pos + 1] if pos + 1 < len(nodes) else len(out)
        with np.errstate(all="ignore"):
            try:
                D = np.dot(S_nodes[pos], np.linalg.inv(out[k0]))
            except np.linalg.LinAlgError:
                continue
        if not np.isfinite(D).all():
            continue
        for k in range(k0, k1):
            if np.isfinite(out[k]).all():
                T = np.dot(D, out[k])
                out[k] = T / T[2, 2]
    return out


# ---- the drivers -----------------------------------------------------------------------------------------------------------------------
def _align_arguments(superposition, resize_info, model, iters, stride, min_inliers, min_gap, min_overlap, max_partners, inlier_thr,
                     huber_delta, fixed, ingest):
    """The refusals of align_superposition, before the capture is opened or the device touched"""
    check_ingest(ingest)
    if model not in BASIS:
        raise ValueError("model must be one of %s" % ", ".join(MODELS))
    iters, stride, min_inliers = _whole(iters, 0, "iters"), _whole(stride, 1, "stride"), _whole(min_inliers, 1, "min_inliers")
    for v, name in ((inlier_thr, "inlier_thr"), (huber_delta, "huber_delta")):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v < 0:
            raise ValueError("%s must be a number of at least 0" % name)
    w, h = int(resize_info["w"]), int(resize_info["h"])
    if w < 1 or h < 1:
        raise ValueError("resize_info must hold a positive w and h")
    keys = [k for k in superposition if k != "resize_info"]
    nodes = list(range(0, len(keys), stride))
    if nodes and not 0 <= _whole(fixed, 0, "fixed") < len(nodes):
        raise ValueError("fixed must name one of the %d node frames" % len(nodes))
    if len(nodes) > MAX_NODES:
        raise ValueError("stride = %d makes %d node frames, more than the %d the dense host solve takes: raise stride"
                         % (stride, len(nodes), MAX_NODES))
    if len(nodes) * w * h * 3 > NODE_BYTES_BUDGET:
        raise ValueError("stride = %d keeps %d node frames of %d x %d on the device, %d bytes, more than the budget of %d: raise stride"
                         % (stride, len(nodes), w, h, len(nodes) * w * h * 3, NODE_BYTES_BUDGET))
    node_sup = {keys[k]: superposition[keys[k]] for k in nodes}
    edges, loops = loop_candidates(node_sup, resize_info, min_gap, min_overlap, max_partners) if nodes else ([], {})
    return keys, nodes, w, h, edges, loops


def match_edges(ctx, node_frames, edges, chunk=PAIRS_PER_CALL):
    """node_frames: CUDA uint8 [nnodes,h,w,3]; edges [(i, j)] over the nodes -> (rows f32[nedges,cap,4], counts i32[nedges], H f64
    [nedges,9], status i32[nedges]) on the device: each pair laid out (prev, cur) = (frame j, frame i) and matched by
    pair_homography_batch (independent pairs, ORB), `chunk` pairs per call; the rows are batch_static_rows' (a in frame i, b in
    frame j), H the pair's matrix (a onto b) and status its final status."""
    import torch
    from ._lib import MODE_INDEPENDENT_PAIRS
    dev, ne = node_frames.device, len(edges)
    cap = ctx.lib.evh_orb_capacity(ctx.h)
    rows = torch.zeros((ne, cap, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros(ne, dtype=torch.int32, device=dev)
    front = torch.zeros(ne, dtype=torch.int32, device=dev)
    H = torch.zeros((ne, 9), dtype=torch.float64, device=dev)
    status = torch.full((ne,), -1, dtype=torch.int32, device=dev)
    order = torch.tensor([f for i, j in edges for f in (j, i)], dtype=torch.int64, device=dev)
    for first in range(0, ne, chunk):
        n = min(chunk, ne - first)
        frames = node_frames.index_select(0, order[2 * first:2 * (first + n)]).contiguous()
        ctx.pair_homography_batch(frames, n, MODE_INDEPENDENT_PAIRS, H[first:first + n], status[first:first + n])
        ctx.batch_static_rows(0, n, rows[first:first + n], counts[first:first + n], front[first:first + n])
        ctx.order_torch_after()
    return rows, counts, H, status


def align_superposition(capture, superposition, resize_info, model="homography", iters=10, stride=1, min_inliers=20, min_gap=8,
                        min_overlap=0.3, max_partners=4, inlier_thr=3.0, huber_delta=0.0, fixed=0, chunk_frames=32, ingest="auto",
                        normal=None):
    """The whole chain aligned at once.  The video is read as registration.registration_report reads it (frames.FrameReader,
    frames.DeviceLadder, at the working size of resize_info); every stride-th frame is a NODE and stays on the device (at most
    MAX_NODES of them and NODE_BYTES_BUDGET bytes, else a ValueError naming stride); loop_candidates of the nodes' matrices are matched
    (match_edges); an edge is kept when its status is OK and at least min_inliers of its rows lie within inlier_thr of its own
    pair matrix (evh_graph_normal's gate); the kept edges must connect every node to node `fixed` (check_connected); solve_graph
    runs on the plane normalised by plane_normalisation, huber_delta (plane pixels, 0: plain least squares) scaled with it;
    frames between two nodes follow the node before them (spread_corrections).  iters = 0 matches, reports and changes nothing.
    normal: in place of the device call, normal(S, edges, rows, counts, H_edge, inlier_thr, huber_delta) -> (sums, info) on host
    arrays (the restatement of tests/graph_checks.py).
    -> ({frame_no: S'_k f64[3,3]}, report: edges_tried, edges_kept, loop_edges {frame_no: [frame_no]}, loop_edges_kept, used per kept
    edge, cost_before, cost_after, steps, accepted, model, nodes)."""
    import torch
    keys, nodes, w, h, edges, loops = _align_arguments(superposition, resize_info, model, iters, stride, min_inliers, min_gap,
                                                       min_overlap, max_partners, inlier_thr, huber_delta, fixed, ingest)
    if not keys:
        return {}, {"edges_tried": [], "edges_kept": []}
    S = np.stack([entry_matrix(superposition[k]) for k in keys])
    reader = FrameReader(capture, ingest)
    first = reader.first
    if not reader.planes and (first.ndim not in (2, 3) or (first.ndim == 3 and first.shape[2] != 3)):
        raise ValueError("frames must be BGR [h,w,3] or gray [h,w]")
    ctx = runtime.get_context(w, h, nframes=2 * PAIRS_PER_CALL)
    dev = runtime.device()
    chunk = max(1, min(int(chunk_frames), len(keys), runtime.STAGING_BYTES_PER_BUFFER // max(first.nbytes, 1)))
    ladder = DeviceLadder(dev, chunk, reader.planes, (reader.w0, reader.h0), (w, h), bgr=True, gray3=True)
    node_frames = torch.empty((len(nodes), h, w, 3), dtype=torch.uint8, device=dev)
    seen = 0
    for start, frames in reader.chunks(chunk, 0, len(keys)):
        src = ladder(ctx, torch.from_numpy(frames).to(dev))[1]
        ctx.order_torch_after()
        for k in range(start, start + len(frames)):
            if k % stride == 0:
                node_frames[k // stride] = src[k - start]
        seen = start + len(frames)
    if seen < len(keys):
        raise ValueError("the capture holds fewer frames than the dictionary")
    report = {"model": model, "nodes": [keys[k] for k in nodes], "edges_tried": [(keys[nodes[i]], keys[nodes[j]]) for i, j in edges],
              "loop_edges": {keys[nodes[i]]: [keys[nodes[j]] for j in js] for i, js in loops.items()}}
    Sn = S[nodes]
    if not edges:
        report.update(edges_kept=[], loop_edges_kept={}, used=[], cost_before=None, cost_after=None, steps=0, accepted=0)
        return dict(zip(keys, S)), report
    rows, counts, H, status = match_edges(ctx, node_frames, edges)
    N, scale = plane_normalisation({keys[k]: superposition[keys[k]] for k in nodes}, resize_info)
    e_all = np.asarray(edges, np.int32)

    if normal is None:
        d_edges = torch.from_numpy(e_all).to(dev)

        def run(mats, which=None):
            sel = (lambda t: t) if which is None else (lambda t: t.index_select(0, which).contiguous())
            sums, info = graph_normal(ctx, mats, sel(d_edges), sel(rows), sel(counts), None, sel(H), inlier_thr, huber_delta * scale)
            ctx.order_torch_after()
            return sums.cpu().numpy(), info.cpu().numpy()
    else:
        h_rows, h_counts, h_H = rows.cpu().numpy(), counts.cpu().numpy(), H.cpu().numpy()

        def run(mats, which=None):
            sel = (lambda a: a) if which is None else (lambda a: a[which.cpu().numpy()])
            return normal(mats, sel(e_all), sel(h_rows), sel(h_counts), sel(h_H), inlier_thr, huber_delta * scale)[:2]
    Nn = np.stack([np.dot(N, m) for m in Sn])
    _, info = run(Nn)
    keep = keep_edges(status.cpu().numpy(), info, min_inliers)
    kept = [e for e, k in zip(edges, keep) if k]
    report["edges_kept"] = [(keys[nodes[i]], keys[nodes[j]]) for i, j in kept]
    report["used"] = [int(u) for u, k in zip(info[:, 0], keep) if k]
    report["loop_edges_kept"] = {}
    for i, j in kept:
        if i - j > 1:
            report["loop_edges_kept"].setdefault(keys[nodes[i]], []).append(keys[nodes[j]])
    try:
        check_connected(kept, len(nodes), fixed)
    except ValueError as e:                                    # name the consecutive edges that were dropped: they are what breaks a chain
        h_status = status.cpu().numpy()
        thin = ["(%s, %s): status %d, %d inliers" % (keys[nodes[i]], keys[nodes[j]], h_status[e_], info[e_, 0])
                for e_, (i, j) in enumerate(edges) if i - j == 1 and not keep[e_]]
        raise ValueError("%s; min_inliers = %d dropped %d consecutive edges, the first: %s" % (e, min_inliers, len(thin), "; ".join(thin[:6])))
    which = torch.from_numpy(np.nonzero(keep)[0].astype(np.int64)).to(dev)
    solved, rep = solve_graph(Sn, evaluator(lambda mats: run(mats, which), kept), model, iters, fixed, N)
    report.update(cost_before=rep["cost_before"], cost_after=rep["cost_after"], steps=rep["steps"], accepted=rep["accepted"])
    out = spread_corrections(S, nodes, solved) if int(iters) > 0 else S
    return dict(zip(keys, out)), report


def aligned_homography_dict(capture_factory, superposition, resize_info, threshold=16, chunk_frames=32, ingest="auto", **align):
    """align_superposition, its matrices turned into a dictionary in the reference's format, and the score of both.
    capture_factory() opens the video; it is called three times.  H'_k = S'_k . S'_{k-1}^-1 / [2][2], None where that is not finite.
    -> {"homography": {frame_no: {"H": ...}} for every entry but the first, "superposition": {frame_no: S'}, "report":
    align_superposition's plus "report_before" / "report_after": registration.registration_report of the
    dictionary handed in and of the aligned one}"""
    from . import registration
    if isinstance(threshold, bool) or int(threshold) != threshold or not 0 <= int(threshold) <= 255:
        raise ValueError("threshold must be an integer in 0..255")
    sup, report = align_superposition(capture_factory(), superposition, resize_info, chunk_frames=chunk_frames, ingest=ingest, **align)
    keys = list(sup)
    hd = {}
    for k0, k1 in zip(keys, keys[1:]):
        H = None
        with np.errstate(all="ignore"):
            try:
                H = np.dot(sup[k1], np.linalg.inv(sup[k0]))
                H = H / H[2, 2]
            except np.linalg.LinAlgError:
                H = None
        hd[k1] = {"H": H.tolist() if H is not None and np.isfinite(H).all() else None}
    report["report_before"] = registration.registration_report(capture_factory(), superposition, resize_info, threshold, chunk_frames, ingest)
    report["report_after"] = registration.registration_report(capture_factory(), sup, resize_info, threshold, chunk_frames, ingest)
    return {"homography": hd, "superposition": sup, "report": report}
