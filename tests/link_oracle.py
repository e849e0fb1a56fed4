"""NumPy / scipy / plain-Python oracles of the distance-based linker
("Distance-based linker"), integers throughout.

centroids(cols): the quantised centroids from region_oracle's record columns.
matrix(...): the explicit P x (C + P) matrix of one frame pair, absent entries
    at P g2 + 1 (more than any feasible total, so scipy never takes one where a
    feasible assignment exists -- and one always does).
scipy_pair(M): (total, col4row) by scipy.optimize.linear_sum_assignment.
unique_optimum(M, col4row): forbids each chosen entry in turn and checks that
    the total rises.
algorithm(M, absent): the algorithm of the definition in plain Python, for
    small cases: (total, col4row).
mothers(...), link(...): the per-record outputs of the whole table.
assemble(...): the track assembly.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment


def centroids(cols):
    a = np.asarray(cols["area"], np.int64)
    qy = (32 * np.asarray(cols["sum_y"], np.int64) + a) // (2 * a)
    qx = (32 * np.asarray(cols["sum_x"], np.int64) + a) // (2 * a)
    return qy, qx


def gate_q(gate):
    return int(np.floor(16.0 * gate + 0.5))


def distances(qy, qx, p, c):
    """d(i, j) of previous records p (slice) and current records c (slice)."""
    dy = qy[p].astype(np.int64)[:, None] - qy[c].astype(np.int64)[None, :]
    dx = qx[p].astype(np.int64)[:, None] - qx[c].astype(np.int64)[None, :]
    return dy * dy + dx * dx


def matrix(d, g2):
    """The explicit matrix of a pair from its (P, C) distances: (M, absent)."""
    P, C = d.shape
    absent = P * g2 + 1
    M = np.full((P, C + P), absent, np.int64)
    M[:, :C] = np.where(d <= g2, d, absent)
    M[np.arange(P), C + np.arange(P)] = g2
    return M, absent


def scipy_pair(M):
    if M.shape[0] == 0:
        return 0, np.zeros(0, np.int64)
    r, c = linear_sum_assignment(M)
    return int(M[r, c].sum()), c.astype(np.int64)


def unique_optimum(M, col4row, absent):
    total = int(M[np.arange(len(col4row)), col4row].sum())
    for i, j in enumerate(col4row):
        T = M.copy()
        T[i, j] = absent
        if scipy_pair(T)[0] <= total:
            return False
    return True


def algorithm(M, absent):
    """Shortest augmenting paths in the form of Crouse 2016: rows ascending,
    the strict update, and the next column among the unscanned columns of least
    distance (a) unassigned before assigned, (b) lowest index."""
    P, N = len(M), (len(M[0]) if len(M) else 0)
    INF = None
    u = [0] * P
    v = [0] * N
    col4row = [-1] * P
    row4col = [-1] * N
    path = [-1] * N
    for cur in range(P):
        shortest = [INF] * N
        SR, SC = set(), set()
        minval, i, sink = 0, cur, -1
        while sink < 0:
            SR.add(i)
            best = None
            for j in range(N):
                if j in SC:
                    continue
                if M[i][j] != absent:
                    r = minval + int(M[i][j]) - u[i] - v[j]
                    if shortest[j] is INF or r < shortest[j]:
                        shortest[j] = r
                        path[j] = i
                if shortest[j] is INF:
                    continue
                key = (shortest[j], row4col[j] >= 0, j)
                if best is None or key < best:
                    best = key
            minval, _, j = best
            SC.add(j)
            if row4col[j] < 0:
                sink = j
            else:
                i = row4col[j]
        u[cur] += minval
        for r in SR:
            if r != cur:
                u[r] += minval - shortest[col4row[r]]
        for j in SC:
            v[j] -= minval - shortest[j]
        j = sink
        while True:
            r = path[j]
            row4col[j] = r
            col4row[r], j = j, col4row[r]
            if r == cur:
                break
    total = sum(int(M[i][col4row[i]]) for i in range(P))
    return total, np.array(col4row, np.int64)


def outputs(offsets, qy, qx, f, col4row, dq):
    """prev / dist / mother of the current frame f + 1 of pair f from col4row."""
    o0, o1, o2 = (int(offsets[f + k]) for k in range(3))
    P, C = o1 - o0, o2 - o1
    d = distances(qy, qx, slice(o0, o1), slice(o1, o2))
    prev = np.full(C, -1, np.int64)
    dist = np.full(C, -1, np.int64)
    mother = np.full(C, -1, np.int64)
    linked = np.zeros(P, bool)
    for i, j in enumerate(col4row):
        if j < C:
            prev[j], dist[j], linked[i] = o0 + i, d[i, j], True
    if dq > 0:
        for j in range(C):
            if prev[j] >= 0:
                continue
            ok = linked & (d[:, j] <= dq * dq)
            if ok.any():
                cand = np.where(ok, d[:, j], np.iinfo(np.int64).max)
                mother[j] = o0 + int(np.argmin(cand))      # argmin: the first, so the lowest i
    return prev, dist, mother


def link(offsets, cols, gate, division_gate=0.0, solver="scipy", unique_pairs=None):
    """The oracle's outputs for a whole table: dict(prev, dist, mother,
    pair_total, unique).  solver "scipy": every pair by scipy's assignment;
    unique[f] says whether pair f's optimum is the only one, for the pairs in
    unique_pairs (None = all of them; None in the list where not checked).
    solver "algorithm": every pair by the plain-Python algorithm."""
    n = len(offsets) - 1
    total = int(offsets[-1])
    qy, qx = centroids(cols)
    gq, dq = gate_q(gate), gate_q(division_gate)
    g2 = gq * gq
    prev = np.full(total, -1, np.int64)
    dist = np.full(total, -1, np.int64)
    mother = np.full(total, -1, np.int64)
    pair_total = np.zeros(max(n - 1, 0), np.int64)
    unique = [None] * max(n - 1, 0)
    for f in range(n - 1):
        o0, o1, o2 = (int(offsets[f + k]) for k in range(3))
        M, absent = matrix(distances(qy, qx, slice(o0, o1), slice(o1, o2)), g2)
        if solver == "scipy":
            t, c4r = scipy_pair(M)
            if unique_pairs is None or f in unique_pairs:
                unique[f] = unique_optimum(M, c4r, absent)
        else:
            t, c4r = algorithm(M.tolist(), absent)
        pair_total[f] = t
        prev[o1:o2], dist[o1:o2], mother[o1:o2] = outputs(offsets, qy, qx, f, c4r, dq)
    return dict(prev=prev, dist=dist, mother=mother, pair_total=pair_total, unique=unique)


def assemble(offsets, cols, frames, prev, mother, division_min_ratio=0.5, max_children=2):
    """(rows (tracks, 4): id start end parent, ids per record)."""
    n = len(offsets) - 1
    frames = [int(f) for f in frames]
    assert all(b > a for a, b in zip(frames, frames[1:]))
    qy, qx = centroids(cols)
    area = np.asarray(cols["area"], np.int64)
    ids = np.zeros(int(offsets[-1]), np.int64)
    rows = []
    for f in range(n):
        o1, o2 = int(offsets[f]), int(offsets[f + 1])
        parent = {}
        if f > 0 and max_children >= 2:
            succ = {int(prev[r]): r for r in range(o1, o2) if prev[r] >= 0}
            claims = {}
            for r in range(o1, o2):
                if mother[r] >= 0 and int(mother[r]) in succ:
                    claims.setdefault(int(mother[r]), []).append(r)
            for i in sorted(claims):
                k = succ[i]
                ok = [r for r in claims[i]
                      if min(float(area[k]), float(area[r])) / max(float(area[k]), float(area[r])) >= division_min_ratio]
                ok.sort(key=lambda r: (int((qy[i] - qy[r]) ** 2 + (qx[i] - qx[r]) ** 2), r))
                ok = ok[:max_children - 1]
                if ok:
                    for r in [k] + ok:
                        parent[r] = i
        for r in range(o1, o2):
            if r in parent:
                rows.append([len(rows) + 1, frames[f], frames[f], int(ids[parent[r]])])
                ids[r] = len(rows)
            elif f > 0 and prev[r] >= 0:
                ids[r] = ids[prev[r]]
                rows[ids[r] - 1][2] = frames[f]
            else:
                rows.append([len(rows) + 1, frames[f], frames[f], -1])
                ids[r] = len(rows)
    return np.array(rows, np.int64).reshape(-1, 4), ids
