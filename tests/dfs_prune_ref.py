"""The pruned depth-first walker (TEST HELPER, CPU only), the reference of ``SPaRCVecEnv.dfs(prune=...)``
/ sparc_dfs_pruned_device: ``dfs_ref.Walker`` with another ``_forward`` and nothing else changed.  A
node's children are the forward moves whose ``live`` bit is set in ``reach_ref.reach_one`` of the
node's state (the path's points visited, the agent's own among them) and, in the deadline mode, whose
``action_dist`` still fits: node step + action_dist[a] <= max_steps."""
import numpy as np

import dfs_ref
import reach_ref

REACH, DEADLINE = 1, 3


class PrunedWalker(dfs_ref.Walker):
    def __init__(self, p, prefix=(), prune=REACH, **kw):
        assert prune in (REACH, DEADLINE)
        self.prune = prune
        super().__init__(p, prefix, **kw)

    def _forward(self, frm=0):
        key = tuple(self.pts)
        if getattr(self, "_asked", None) != key:                    # the walker asks two or three times per node
            visited = np.zeros((self.X, self.Y), np.uint8)
            for pt in self.pts:
                visited[pt] = 1
            _, self._ad, self._live, _, _ = reach_ref.reach_one(self.p, *self.pts[-1], visited)
            self._asked = key
        ad, live = self._ad, self._live
        step = self.root_step + len(self.pts) - self.root_len
        return [a for a in range(frm, 4) if (live >> a) & 1 and
                (self.prune != DEADLINE or step + int(ad[a]) <= self.max_steps)]


def walk(p, prefix=(), budget=None, **kw):
    """One ``PrunedWalker.run``: the complete pruned walk below ``prefix``, or its first ``budget`` nodes."""
    return PrunedWalker(p, prefix, **kw).run(budget)


_walks = {}


def complete_walks(name, **kw):
    """The traced complete pruned walk from the start of every puzzle of pool ``name`` (cached)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _walks:
        _walks[key] = [PrunedWalker(p, trace=True, **kw).run() for p in dfs_ref.pool(name)]
    return _walks[key]
