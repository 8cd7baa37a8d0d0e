"""A UCT tree search over the CPU restatement of the env (TEST HELPER, CPU only), the reference of
SPaRCVecEnv.mcts / sparc_mcts_device.

Written from the interface's description (include/sparc_gym_amd.h), not from the kernel: the states
are ``oracle.cpu_ref.CpuRefEnv`` objects stepped with its own ``step``, the rollout draws with
``search.rand_pick``, and the scores are numpy float32 scalars, one rounding per operation.

A tree is a list of 16-word nodes: w0 parent | action << 28 | kind << 30; w1-3 visits, wins, losses;
w4-7 child[a] (0 untried, NONE not a child); w8-11 n[a]; w12-15 wins[a].  The children of a node are
its legal actions without the traceback pop; a node that is not inner has none.
"""
import numpy as np

from oracle.cpu_ref import DIRS, CpuRefEnv
from sparc_gym_amd.search import rand_pick

INVALID, DONE, FULL, PENDING, DEAD_END = range(5)
NONE = 0xFFFFFFFF
INNER, TERMINATED, TRUNCATED, DEAD = range(4)
VISITS, WINS, LOSSES, CHILD, N, CHILD_WINS = 1, 2, 3, 4, 8, 12


def pool_entry(p):
    """A processed puzzle as the dict CpuRefEnv takes."""
    return {"x_size": p["x_size"], "y_size": p["y_size"], "start": list(p["start_location"]),
            "target": list(p["target_location"]), "solution_count": p["solution_count"],
            "solution_paths": p["solution_paths"], "gaps": p["obs_array"]["gaps"]}


def code_of(reward):
    """The reward code of a step's reward: +-100 for +-1, +-1 for +-0.01, 0."""
    return int(round(reward * 100))


def clone(env):
    new = object.__new__(CpuRefEnv)
    new.__dict__.update(env.__dict__)
    new.visited = env.visited.copy()
    new.path = [list(pt) for pt in env.path]
    new.loc = list(env.loc)
    return new


def masks(env):
    """(legal, forward): bit a set when action a is legal / legal and not the traceback pop."""
    legal = forward = 0
    for a in env.legal_actions():
        legal |= 1 << a
        if env.visited[env.loc[0] + DIRS[a][0], env.loc[1] + DIRS[a][1]] == 0:
            forward |= 1 << a
    return legal, forward


class Root:
    """The state after ``actions`` from the start of pool entry ``p``; ``pending``: its last step ended
    the episode (no action may follow one that did)."""

    def __init__(self, p, actions=(), traceback=True, max_steps=2000):
        self.env = CpuRefEnv(p, traceback=traceback, max_steps=max_steps)
        self.pending = False
        for a in actions:
            assert not self.pending
            _, term, trunc = self.env.step(int(a))
            self.pending = term or trunc


def new_node(parent, action, kind, forward):
    node = [0] * 16
    node[0] = parent | (action << 28) | (kind << 30)
    for a in range(4):
        node[CHILD + a] = 0 if kind == INNER and (forward >> a) & 1 else NONE
    return node


class Tree:
    """The tree of one root, its winner and what the last ``run`` reported."""

    def __init__(self, root):
        self.root = root
        self.nodes = []
        self.win_steps = NONE
        self.win_actions = None          # the winner's actions from the root
        self.status, self.sims = INVALID, 0

    def array(self, cap=None):
        """The arena of this root: [cap, 16] uint32, zero past the tree."""
        out = np.zeros((len(self.nodes) if cap is None else cap, 16), np.uint32)
        if self.nodes:
            out[:len(self.nodes)] = np.asarray(self.nodes, np.uint64).astype(np.uint32)
        return out

    def run(self, sims, L, cap, ep, ec, seed=0, id_base=0, forward_only=False):
        """``sims`` more simulations; ``id_base`` = id0 + j * 2^32 of root j."""
        ep, ec = np.asarray(ep, np.float32), np.asarray(ec, np.float32)
        T = len(ep)
        assert T >= 2 and len(ec) == T and cap >= 1 and len(self.nodes) <= cap
        self.sims = 0
        root = self.root
        if root.pending:
            self.status = PENDING
            return self
        fwd0 = masks(root.env)[1]
        if fwd0 == 0:
            self.status = DEAD_END
            return self
        nodes = self.nodes
        if not nodes:
            nodes.append(new_node(0, 0, INNER, fwd0))
        tb = root.env.traceback
        for _ in range(sims):
            s = nodes[0][VISITS]
            if s == NONE:
                self.status = FULL
                return self
            env, at, acts, code = clone(root.env), 0, [], 0
            while True:
                node = nodes[at]
                untried = [a for a in range(4) if node[CHILD + a] == 0]
                if untried:
                    if len(nodes) == cap:
                        self.status = FULL      # nothing of this simulation has been written
                        return self
                    a = untried[0]
                    reward, term, trunc = env.step(a)
                    code = code_of(reward)
                    acts.append(a)
                    forward = masks(env)[1]
                    kind = TERMINATED if term else TRUNCATED if trunc else (INNER if forward else DEAD)
                    nodes.append(new_node(at, a, kind, forward))
                    node[CHILD + a] = at = len(nodes) - 1
                    if kind == INNER:
                        for t in range(L):
                            legal, forward = masks(env)
                            mask = forward if (forward_only and tb) else legal
                            if mask == 0 and legal != 0:
                                break
                            a = int(rand_pick(seed, id_base + s, t, mask))
                            reward, term, trunc = env.step(a)
                            code = code_of(reward)
                            acts.append(a)
                            if term or trunc:
                                break
                    break
                pe = ep[min(node[VISITS], T - 1)]
                best, top = None, None
                for a in range(4):
                    if node[CHILD + a] != NONE:
                        n = node[N + a]
                        x = np.float32(node[CHILD_WINS + a]) / np.float32(n) + pe * ec[min(n, T - 1)]
                        assert x.dtype == np.float32
                        if best is None or x > top:
                            best, top = a, x
                reward, term, trunc = env.step(best)
                code = code_of(reward)
                acts.append(best)
                at = node[CHILD + best]
                kind = nodes[at][0] >> 30
                assert (term, trunc) == (kind == TERMINATED, kind == TRUNCATED)   # the step that made it
                if kind != INNER:
                    break
            win, loss = int(code == 100), int(code == -100)
            if win and len(acts) < self.win_steps:
                self.win_steps, self.win_actions = len(acts), list(acts)
            while True:
                node = nodes[at]
                node[VISITS] += 1
                node[WINS] += win
                node[LOSSES] += loss
                if at == 0:
                    break
                parent, a = node[0] & 0x0FFFFFFF, (node[0] >> 28) & 3
                nodes[parent][N + a] += 1
                nodes[parent][CHILD_WINS + a] += win
                at = parent
            self.sims += 1
        self.status = DONE
        return self


def prefixes(pool, M, traceback, max_steps, seed=0):
    """M mid-episode starts on the puzzles of ``pool`` (CpuRefEnv dicts): a list of (puzzle index,
    action list), made by seeded walks over legal moves that stop when the episode ends.  Root j
    is on puzzle (7 j + 3) mod P.  Of every eight, roots 0-4 walk forward (the pop one time in
    eight) for 0-6 steps and stay live; root 5 walks to within two steps of max_steps, so the
    limit truncates inside its tree; root 6 walks until its episode ends (pending); root 7 walks
    forward only until it is walled in (several tries; live without a forward move)."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(M):
        pid = (7 * j + 3) % len(pool)
        kind = j % 8
        want = int(rng.integers(0, 7)) if kind < 5 else max_steps - 2 if kind == 5 else 10 * max_steps
        for attempt in range(40 if kind == 7 else 1):
            env, acts, done = CpuRefEnv(pool[pid], traceback=traceback, max_steps=max_steps), [], False
            while len(acts) < want and not done:
                legal, forward = masks(env)
                mask = forward if forward and (kind == 7 or rng.integers(0, 8) != 0) else legal
                if kind == 7 and forward == 0:
                    break
                if kind == 5 and len(acts) == want - 1 and forward:
                    # do not end on the target or in a corner: the tree below should meet the limit
                    mask = forward
                a = int(rng.choice([a for a in range(4) if (mask >> a) & 1]))
                _, term, trunc = env.step(a)
                acts.append(a)
                done = term or trunc
            if kind != 7 or (not done and masks(env)[1] == 0):
                break
        out.append((pid, acts))
    return out


def search(pool, starts, traceback, max_steps, sims, L, cap, ep, ec, seed=0, id0=0, forward_only=False, trees=None):
    """``sims`` simulations on the tree of every start of ``starts`` (``prefixes``' format): fresh
    trees, or ``trees`` of an earlier call continued.  Returns the list of ``Tree``."""
    if trees is None:
        trees = [Tree(Root(pool[pid], acts, traceback, max_steps)) for pid, acts in starts]
    for j, tree in enumerate(trees):
        tree.run(sims, L, cap, ep, ec, seed, id0 + (j << 32), forward_only)
    return trees


def uct_tables(c=1.0, entries=4096):
    """The default tables of SPaRCVecEnv.mcts, computed here on their own."""
    n = np.maximum(np.arange(entries, dtype=np.float64), 1.0)
    return (c * np.sqrt(np.log(n))).astype(np.float32), (1.0 / np.sqrt(n)).astype(np.float32)
