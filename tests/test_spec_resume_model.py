"""Host model of the speculation's resume rule (ksched_phase2v.h, C): after a
mis-speculation at pod k* (its speculated node Y released, its exact node X
taken), the pods before the first affected one keep their decisions and the
speculation resumes there, from the pointer snapshot of that pod's macro-step.

A later pod q is affected iff Y (>= 0, != X) stands in T_q before q's decided
pointer, or X is newly changed and q's own node is X.  The model mirrors the
walk's state (pointers, per-macro-step snapshots, macro-step numbers kept for
the kept pods, the snapshot-row bound and its fallback to a full restart) and
checks every round against sequential re-speculation from scratch."""
import numpy as np

ROWS = 16   # snapshot rows == pods per batch (the walk: 64 and 64)


class Walk:
    def __init__(self, tops, changed):
        self.T = tops
        self.nb = len(tops)
        self.taken = set(changed)      # the changed bitmap
        self.committed = set(changed)  # nodes of committed slots
        self.ptr = [0] * self.nb
        for q in range(self.nb):
            self._validate(q)
        self.dec = [-1] * self.nb
        self.dptr = [0] * self.nb
        self.mstep = [0] * self.nb
        self.snap = [[0] * self.nb for _ in range(ROWS)]
        self.kept = self.fallbacks = 0

    def _cand(self, q):
        return self.T[q][self.ptr[q]] if self.ptr[q] < len(self.T[q]) else -1

    def _validate(self, q):
        while self._cand(q) >= 0 and self._cand(q) in self.taken:
            self.ptr[q] += 1

    def speculate(self, rs, mi):
        cur = rs
        while cur < self.nb:
            assert mi < ROWS, "snapshot rows exhausted"
            self.snap[mi] = list(self.ptr)
            seen, f = set(), self.nb
            for q in range(cur, self.nb):
                c = self._cand(q)
                if c >= 0 and c in seen:
                    f = q
                    break
                seen.add(c)
            for q in range(cur, f):
                self.dptr[q], self.mstep[q], self.dec[q] = self.ptr[q], mi, self._cand(q)
                if self.dec[q] >= 0:
                    self.taken.add(self.dec[q])
            for q in range(f, self.nb):
                self._validate(q)
            cur, mi = f, mi + 1

    def rollback(self, k, X):
        """Pod k's exact node is X (-1: none); returns the pod the speculation resumed at."""
        nb, Y = self.nb, self.dec[k]
        self.committed |= {d for d in self.dec[:k] if d >= 0}   # the pods before k are committed
        for q in range(k, nb):
            self.taken.discard(self.dec[q])
        new_x = X >= 0 and X not in self.committed
        if X >= 0:
            self.taken.add(X)
            self.committed.add(X)
        self.dec[k] = X
        pos = [-1] * nb
        if Y >= 0 and Y != X:
            for q in range(k + 1, nb):
                # (Y was free at the snapshot of k's macro-step: the scan starts at that pointer)
                lo = self.snap[self.mstep[k]][q]
                head = self.T[q][lo:self.dptr[q]]
                pos[q] = lo + head.index(Y) if Y in head else -1
                assert Y not in self.T[q][:lo]
        aff = [q for q in range(k + 1, nb) if pos[q] >= 0 or (new_x and self.dec[q] == X)]
        q1 = aff[0] if aff else nb
        row = self.mstep[q1 if q1 < nb else k]
        m0 = row + 1
        full = q1 < nb and m0 + (nb - q1) > ROWS
        if full:
            q1, m0, row = k + 1, 0, self.mstep[k]
            self.fallbacks += 1
        self.kept += q1 - (k + 1)
        for q in range(k + 1, q1):
            if self.dec[q] >= 0:
                self.taken.add(self.dec[q])
        for q in range(q1, nb):
            self.ptr[q] = self.snap[row][q]
            if pos[q] >= 0:
                self.ptr[q] = min(self.ptr[q], pos[q])
                if not full:
                    for m in range(self.mstep[k], row + 1):
                        self.snap[m][q] = min(self.snap[m][q], pos[q])
            self._validate(q)
        self.speculate(q1, m0)
        return q1


def sequential(tops, changed, dec, k):
    """Pods after k re-speculated one by one from the state pods <= k left."""
    taken = set(changed) | {d for d in dec[:k + 1] if d >= 0}
    out = []
    for q in range(k + 1, len(tops)):
        d = next((n for n in tops[q] if n not in taken), -1)
        if d >= 0:
            taken.add(d)
        out.append(d)
    return out


def test_resume_equals_sequential_respeculation():
    rng = np.random.Generator(np.random.PCG64(7))
    cases = kept_cases = fallback_cases = 0
    for trial in range(400):
        nb = ROWS
        n_nodes = int(rng.integers(6, 60))
        hot = rng.permutation(n_nodes)
        tops = []
        for q in range(nb):   # top sets that share hot nodes: a noisy copy of one order
            K = int(rng.integers(1, min(n_nodes, nb + 4) + 1))
            order = sorted(range(n_nodes), key=lambda i: i + rng.normal(0, 2.0))
            tops.append([int(hot[i]) for i in order[:K]])
        changed0 = {int(x) for x in rng.choice(n_nodes, size=int(rng.integers(0, 4)), replace=False)}
        w = Walk(tops, changed0)
        w.speculate(0, 0)
        assert w.dec == sequential(tops, changed0, [], -1)
        k = -1
        # (mis-speculations close together, as MostAllocated gives them: the macro-step numbers run up)
        while (k := k + 1 + int(rng.integers(0, 2 if trial % 2 else 5))) < nb:
            Y = w.dec[k]
            u = rng.random()
            later = [d for d in w.dec[k + 1:] if d >= 0]
            if u < 0.15:
                X = Y                                            # the rescan confirms the node
            elif u < 0.45 and w.committed:
                X = int(rng.choice(sorted(w.committed)))         # an existing slot's node
            elif u < 0.65 and later:
                X = int(rng.choice(later))                       # a node a later pod holds
            elif u < 0.75:
                X = -1                                           # no node
            else:
                X = int(rng.integers(0, n_nodes))
            changed_now = set(w.committed)
            k0, f0 = w.kept, w.fallbacks
            w.rollback(k, X)
            cases += 1
            kept_cases += w.kept > k0
            fallback_cases += w.fallbacks > f0
            ref = sequential(tops, changed_now | ({X} if X >= 0 else set()), w.dec[:k] + [X], k)
            assert w.dec[k + 1:] == ref, (trial, k, X, Y)
            for q in range(k + 1, nb):   # the decided pointer stands at the node
                assert (tops[q][w.dptr[q]] if w.dptr[q] < len(tops[q]) else -1) == w.dec[q]
    assert cases > 1000 and kept_cases > 0 and fallback_cases > 0, (cases, kept_cases, fallback_cases)
