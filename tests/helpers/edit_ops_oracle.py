"""Oracle of the edit alignment (include/lasr.h lasr_edit_align_batch): the full-matrix Levenshtein DP and the canonical
trace-back, in plain Python over lists of units.

D[i][j] = distance of the first i hypothesis units to the first j reference units.  Walking back from (n_hyp, n_ref) to (0, 0),
at every cell the first that applies:
  1. diagonal:  i > 0, j > 0 and D[i-1][j-1] + (h_i != r_j) == D[i][j]   -> HIT (0) or SUB (1)
  2. deletion:  j > 0 and D[i][j-1] + 1 == D[i][j]                        -> DEL (2), a reference unit with no hypothesis unit
  3. insertion: D[i-1][j] + 1 == D[i][j]                                  -> INS (3), a hypothesis unit with no reference unit
The script is returned forwards."""
HIT, SUB, DEL, INS = 0, 1, 2, 3


def matrix_np(h, r):
    """the same matrix a row at a time in numpy, for the long cases (2048 x 2048 cells take seconds in plain Python):
    cur[j] = min(up[j] + 1, up[j-1] + cost, cur[j-1] + 1) = j + min_{k <= j}(t[k] - k) with t = the first two terms and
    t[0] = cur[0] = i.  tests/test_host_edit_ops.py holds it to matrix() cell for cell."""
    import numpy as np
    ids = {}
    hv = np.array([ids.setdefault(u, len(ids)) for u in h], dtype=np.int64)
    rv = np.array([ids.setdefault(u, len(ids)) for u in r], dtype=np.int64)
    cols = np.arange(len(r) + 1, dtype=np.int64)
    D = [cols.copy()]
    for i in range(1, len(h) + 1):
        up = D[-1]
        t = np.empty(len(r) + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(up[1:] + 1, up[:-1] + (rv != hv[i - 1]))
        D.append(cols + np.minimum.accumulate(t - cols))
    return D


def matrix(h, r):
    return matrix_np(h, r) if len(h) * len(r) > 1 << 16 else matrix_py(h, r)


def matrix_py(h, r):
    nh, nr = len(h), len(r)
    D = [[0] * (nr + 1) for _ in range(nh + 1)]
    for i in range(nh + 1):
        D[i][0] = i
    for j in range(nr + 1):
        D[0][j] = j
    for i in range(1, nh + 1):
        for j in range(1, nr + 1):
            D[i][j] = min(D[i - 1][j - 1] + (h[i - 1] != r[j - 1]), D[i][j - 1] + 1, D[i - 1][j] + 1)
    return D


def script(h, r):
    """(distance, forward script) of hypothesis units h against reference units r"""
    D = matrix(h, r)
    ops = []
    i, j = len(h), len(r)
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1][j - 1] + (h[i - 1] != r[j - 1]) == D[i][j]:
            ops.append(HIT if h[i - 1] == r[j - 1] else SUB)
            i, j = i - 1, j - 1
        elif j > 0 and D[i][j - 1] + 1 == D[i][j]:
            ops.append(DEL)
            j -= 1
        else:
            assert i > 0 and D[i - 1][j] + 1 == D[i][j]
            ops.append(INS)
            i -= 1
    ops.reverse()
    return D[len(h)][len(r)], ops


def counts(ops):
    """[hits, substitutions, deletions, insertions]"""
    return [sum(1 for o in ops if o == k) for k in range(4)]


def words(tokens, space_id):
    """str.split() over token ids: maximal runs of non-space tokens, as tuples; space_id < 0: every token is its own unit"""
    if space_id < 0:
        return [int(t) for t in tokens]
    out, cur = [], []
    for t in tokens:
        if int(t) == space_id:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(int(t))
    if cur:
        out.append(tuple(cur))
    return out


def replay(h, r, ops):
    """walk the script over both sequences: True when it consumes both exactly and marks hits exactly where the units are equal"""
    i = j = 0
    for o in ops:
        if o in (HIT, SUB):
            if i >= len(h) or j >= len(r) or (h[i] == r[j]) != (o == HIT):
                return False
            i, j = i + 1, j + 1
        elif o == DEL:
            if j >= len(r):
                return False
            j += 1
        elif o == INS:
            if i >= len(h):
                return False
            i += 1
        else:
            return False
    return i == len(h) and j == len(r)


def align_batch(hyp, hyp_lens, ref, ref_lens, space_id):
    """rows of token ids (any 2-D indexable) with their lengths, clamped to the row widths -> per utterance
    (dist, ref_units, counts, script, hyp units, ref units)"""
    out = []
    for b in range(len(hyp_lens)):
        nh = max(0, min(int(hyp_lens[b]), len(hyp[b])))
        nr = max(0, min(int(ref_lens[b]), len(ref[b])))
        h = words([int(t) for t in hyp[b][:nh]], space_id)
        r = words([int(t) for t in ref[b][:nr]], space_id)
        d, ops = script(h, r)
        out.append((d, len(r), counts(ops), ops, h, r))
    return out


def confusion(results, n_classes):
    """the (n_classes + 1)^2 matrix of token-mode results: [reference label][hypothesis label], index n_classes = none; an op
    that involves a token id outside [0, n_classes) is left out"""
    M = [[0] * (n_classes + 1) for _ in range(n_classes + 1)]
    for _, _, _, ops, h, r in results:
        i = j = 0
        for o in ops:
            lh = n_classes if o == DEL else h[i]
            lr = n_classes if o == INS else r[j]
            ok_h = o == DEL or 0 <= lh < n_classes
            ok_r = o == INS or 0 <= lr < n_classes
            if ok_h and ok_r:
                M[lr][lh] += 1
            i, j = i + (o != DEL), j + (o != INS)
    return M
