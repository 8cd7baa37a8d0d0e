"""One-ply expansion of state records on the GPU (SPaRCVecEnv.expand, sparc_expand_device).

Child (j, a) must be byte for byte the record of restore(record j) -> one step(a) -> snapshot,
so the yardstick is that composed path on a second context of 4 * M envs, and, independently of
the code under test, the C oracle stepped from the copied structs.  Standing configuration of
test_gpu_snapshot.py: 300 parents give 1,200 children = four full workgroups of 256 and a ragged
one of 176 whose last wave has 48 lanes."""
import numpy as np
import pytest

from test_gpu_parity import POOLS
from test_gpu_snapshot import N, STANDING, _arrays, _assert_interesting, _oracle, _same, _standing, _vec, _warm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = ["next_step", "none"]


def _S(name, tb, n=N):
    S = _standing(name, tb, n)
    if n >= N:
        _assert_interesting(S)
    return S


def _ctx(S, mode):
    """A context at the snapshot point whose autoreset is `mode`.  autoreset belongs to the
    context, not to the state: for "none" the standing state (pending envs, envs past an
    autoreset) is restored into a context without autoreset, where pending parents step past the
    end as the reference does."""
    v = _warm(S)
    if mode == S["autoreset"]:
        return v
    w = _vec(S, autoreset=mode)
    w.restore(v.snapshot())
    return w


def _composed(S, snap, mode="next_step"):
    """The yardstick: a context of 4 * M envs, restore with src = j // 4, ONE step with action
    j % 4, snapshot.  Returns its records, reward codes, flags [4M], the parents' legal masks [M],
    and the context (restored again, not stepped) for a second opinion through rollout."""
    M4 = 4 * len(snap)
    src = np.arange(M4) // 4
    acts = torch.from_numpy((np.arange(M4) % 4).astype(np.uint8)).cuda()
    c = _vec(S, n=M4, autoreset=mode)
    _, info = c.restore(snap, src=src)
    rew = torch.empty(M4, dtype=torch.int8, device="cuda")
    flags = torch.empty(M4, dtype=torch.uint8, device="cuda")
    c.core.step_device(acts.data_ptr(), rew.data_ptr(), flags.data_ptr())
    rec = c.snapshot().records.cpu().numpy()
    c.restore(snap, src=src)
    return dict(records=rec, code=rew.cpu().numpy(), flags=flags.cpu().numpy(),
                legal=info["legal_mask"].cpu().numpy()[::4], ctx=c, acts=acts)


def _check_against(out, ref):
    M = len(ref["legal"])
    assert len(out["children"]) == 4 * M and out["children"].records.is_cuda
    assert out["reward_code"].shape == (M, 4) and out["reward_code"].dtype == torch.int8
    assert out["flags"].shape == (M, 4) and out["flags"].dtype == torch.uint8
    assert np.array_equal(out["children"].records.cpu().numpy(), ref["records"])
    assert np.array_equal(out["reward_code"].cpu().numpy().reshape(-1), ref["code"])
    assert np.array_equal(out["flags"].cpu().numpy().reshape(-1), ref["flags"])
    assert np.array_equal(out["legal_mask"].cpu().numpy(), ref["legal"])


# ----------------------------------------------------------------------------- 1. the step path
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,tb", STANDING)
def test_children_equal_restore_step_snapshot(on_gpu, name, tb, mode):
    S = _S(name, tb)
    v = _ctx(S, mode)
    before = _arrays(v)
    snap = v.snapshot()
    out = v.expand(snap)
    ref = _composed(S, snap, mode)
    _check_against(out, ref)
    # the same step through the rollout kernels, on a fresh restore
    c = ref["ctx"]
    ro = c.rollout(1, ref["acts"][None].contiguous())
    assert np.array_equal(ro["reward_code"].cpu().numpy()[0], ref["code"])
    assert np.array_equal(ro["flags"].cpu().numpy()[0], ref["flags"])
    assert np.array_equal(c.snapshot().records.cpu().numpy(), ref["records"])
    v.core.sync()
    _same(_arrays(v), before)
    # the cases the header documents, present in this configuration
    f, legal = ref["flags"].reshape(N, 4), ref["legal"]
    pending = S["state"]["pending"] != 0
    assert pending.any() and not pending.all()
    if mode == "next_step":
        assert ((f & 64) != 0).all(1)[pending].all() and not ((f & 64) != 0).any(1)[~pending].any()
        rec = ref["records"].reshape(N, 4, -1)
        assert (rec[pending] == rec[pending][:, :1]).all()
    else:
        assert not (f & 64).any()
    assert (((legal[:, None] >> np.arange(4)) & 1) == 0)[~pending].any()      # illegal actions are stepped too


# ----------------------------------------------------------------------------- 2. the C oracle
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,tb", STANDING)
def test_codes_flags_and_legal_mask_equal_the_oracle(on_gpu, name, tb, mode):
    S = _S(name, tb)
    v = _ctx(S, mode)
    out = v.expand()
    o = _oracle(S, src=np.arange(4 * N) // 4, autoreset=mode, n=4 * N)
    ro, fo = o.rollout(1, (np.arange(4 * N) % 4).astype(np.uint8)[None])
    assert np.array_equal(out["reward_code"].cpu().numpy().reshape(-1), ro[0])
    assert np.array_equal(out["flags"].cpu().numpy().reshape(-1), fo[0])
    assert np.array_equal(out["legal_mask"].cpu().numpy(), S["legal"])


# ----------------------------------------------------------------------------- 3. chained
@pytest.mark.parametrize("name,tb", STANDING)
def test_records_written_by_expand_are_valid_parents(on_gpu, name, tb):
    T = 32
    S = _S(name, tb)
    acts = np.random.default_rng(5).integers(0, 4, (T, N)).astype(np.uint8)
    ro, fo = _oracle(S).rollout(T, acts)
    v = _warm(S)
    snap = cur = v.snapshot()
    rows = torch.arange(N, device="cuda")
    a_dev = torch.from_numpy(acts.astype(np.int64)).cuda()
    codes, flags = [], []
    for t in range(T):
        out = v.expand(cur)
        codes.append(out["reward_code"][rows, a_dev[t]])
        flags.append(out["flags"][rows, a_dev[t]])
        cur = out["children"].select(4 * rows + a_dev[t])
    assert np.array_equal(torch.stack(codes).cpu().numpy(), ro)
    assert np.array_equal(torch.stack(flags).cpu().numpy(), fo)
    c = _vec(S)
    c.restore(snap)
    c.rollout(T, torch.from_numpy(acts).cuda())
    assert np.array_equal(cur.records.cpu().numpy(), c.snapshot().records.cpu().numpy())
    v.core.sync()


# ----------------------------------------------------------------------------- 4. sizes
@pytest.mark.parametrize("M", [1, 65])
def test_sizes(on_gpu, M):
    """65 parents: 260 children, 4 lanes past a workgroup boundary."""
    S = _S("7x7_full", True)
    v = _warm(S)
    snap = v.snapshot().select(np.arange(M) * 3 % N)
    assert len(snap) == M
    _check_against(v.expand(snap), _composed(S, snap))


def test_more_parents_than_envs(on_gpu):
    """M is independent of num_envs: an 8-env context expands 300 records of another context,
    and 20 records of its own envs (envs=[...]); it needs its tables only, not even a reset."""
    S, S8 = _S("mixed_5_11", True), _S("mixed_5_11", True, 8)
    snap = _warm(S).snapshot()
    ref = _composed(S, snap)
    _check_against(_vec(S8).expand(snap), ref)                # never reset
    v8 = _warm(S8)
    before = _arrays(v8)
    _check_against(v8.expand(snap), ref)
    envs = [3, 1, 7, 7, 0, 2, 5, 6, 4, 3, 3, 1, 0, 7, 6, 5, 4, 2, 1, 0]
    _check_against(v8.expand(envs=envs), _composed(S8, v8.snapshot(envs=envs)))
    with pytest.raises(ValueError):
        v8.expand(snap, envs=envs)
    _same(_arrays(v8), before)


@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("15x15", False)])
def test_host_form_equals_device_form(on_gpu, name, tb):
    S = _S(name, tb)
    v = _warm(S)
    snap = v.snapshot()
    out = v.expand(snap)
    children, code, flags, pflags = v.core.expand_host(snap.info, snap.numpy())
    assert np.array_equal(children, out["children"].records.cpu().numpy())
    assert np.array_equal(code, out["reward_code"].cpu().numpy())
    assert np.array_equal(flags, out["flags"].cpu().numpy())
    assert np.array_equal((pflags >> 2) & 15, out["legal_mask"].cpu().numpy())
    assert ((pflags & 0xC3) == 0).all()


# ----------------------------------------------------------------------------- 5. refused input
@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("mixed_5_11", False)])
def test_damaged_parents_are_refused_on_the_device(on_gpu, name, tb):
    """The kernel compares before it indexes: a zeroed record, one whose puzzle field holds P and
    one with len 0 get zeroed children; the sync after reports it once; all others are as in the
    undamaged run."""
    from sparc_gym_amd.snapshot import Snapshot
    S = _S(name, tb)
    v = _warm(S)
    snap = v.snapshot()
    good = v.expand(snap)
    v.core.sync()
    rec = snap.records.clone()
    k_zero, k_pid, k_len = 5, 130, 299          # the last one sits in the ragged wave
    P = len(S["proc"])
    rec[k_zero] = 0
    rec[k_pid, 12:16] = torch.tensor(list(int(P).to_bytes(4, "little")), dtype=torch.uint8, device="cuda")
    rec[k_len, 2] = 0
    out = v.expand(Snapshot(rec, snap.info))       # completes
    with pytest.raises(ValueError, match="expand"):
        v.core.sync()
    v.core.sync()                                  # the error is reported once
    bad = np.zeros(N, bool)
    bad[[k_zero, k_pid, k_len]] = True
    ch = out["children"].records.cpu().numpy().reshape(N, 4, -1)
    assert (ch[bad] == 0).all()
    assert (out["reward_code"].cpu().numpy()[bad] == 0).all() and (out["flags"].cpu().numpy()[bad] == 0).all()
    assert (out["legal_mask"].cpu().numpy()[bad] == 0).all()
    assert np.array_equal(ch[~bad], good["children"].records.cpu().numpy().reshape(N, 4, -1)[~bad])
    for k in ("reward_code", "flags", "legal_mask"):
        assert np.array_equal(out[k].cpu().numpy()[~bad], good[k].cpu().numpy()[~bad]), k
    # a zeroed child is no parent either
    again = v.expand(out["children"].select([4 * k_pid + 2, 4 * k_pid + 3]))
    with pytest.raises(ValueError, match="expand"):
        v.core.sync()
    v.core.sync()
    assert (again["children"].records == 0).all() and (again["legal_mask"] == 0).all()
    assert (again["flags"] == 0).all() and (again["reward_code"] == 0).all()


@pytest.mark.parametrize("what", ["table_hash", "traceback"])
def test_header_mismatch_is_rejected(on_gpu, what):
    from sparc_gym_amd.puzzles import pack_table, process_puzzles
    from sparc_gym_amd import synthetic
    S = _S("7x7_full", True)
    s = _warm(S).snapshot()
    if what == "table_hash":       # the same pool with one puzzle exchanged
        proc = list(S["proc"])
        proc[17] = process_puzzles(synthetic.make_puzzles(1, seed=99, **POOLS["7x7_full"]))[0]
        v = _vec(S, processed=proc, table=pack_table(proc))
    else:
        v = _vec(S, traceback=False)
    with pytest.raises(ValueError, match=what):
        v.expand(s)
    children = torch.empty((4 * N, s.info.record_bytes), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=what):          # the library's own check
        v.core.expand_device(s.info, s.records.data_ptr(), N, children.data_ptr())
    v.core.sync()


def test_bad_pointers_are_rejected_on_the_host(on_gpu):
    S = _S("7x7_full", True)
    v = _warm(S)
    s = v.snapshot()
    rb = s.info.record_bytes
    children = torch.empty(4 * N * rb + 16, dtype=torch.uint8, device="cuda")
    shifted = torch.empty(N * rb + 16, dtype=torch.uint8, device="cuda")
    shifted[8:8 + N * rb] = s.records.reshape(-1)
    assert shifted.data_ptr() % 16 == 0 and children.data_ptr() % 16 == 0
    with pytest.raises(ValueError, match="aligned"):
        v.core.expand_device(s.info, shifted.data_ptr() + 8, N, children.data_ptr())
    with pytest.raises(ValueError, match="aligned"):
        v.core.expand_device(s.info, s.records.data_ptr(), N, children.data_ptr() + 8)
    with pytest.raises(ValueError, match="children"):
        v.core.expand_device(s.info, s.records.data_ptr(), N, None)
    with pytest.raises(ValueError, match="records"):
        v.core.expand_device(s.info, None, N, children.data_ptr())
    for M in (0, 2**29):
        with pytest.raises(ValueError, match="M must"):
            v.core.expand_device(s.info, s.records.data_ptr(), M, children.data_ptr())
    v.core.sync()


# ----------------------------------------------------------------------------- Snapshot.select / cat
def test_select_and_cat(on_gpu):
    from sparc_gym_amd.snapshot import Snapshot
    S = _S("7x7_full", True)
    s = _warm(S).snapshot()
    r = s.records.cpu().numpy()
    idx = np.array([7, 7, 0, 299, 12])
    mask = np.arange(N) % 7 == 0
    for snap in (s, s.cpu(), Snapshot(r, s.info)):
        for i in (idx, idx.tolist(), torch.from_numpy(idx), torch.from_numpy(idx).to(torch.int32)):
            got = snap.select(i)
            assert got.is_host == snap.is_host and np.array_equal(got.numpy(), r[idx])
        for m in (mask, torch.from_numpy(mask)):
            assert np.array_equal(snap.select(m).numpy(), r[mask])
        with pytest.raises(ValueError):
            snap.select(np.array([0.5]))
        with pytest.raises(ValueError):
            snap.select(mask[:5])
    both = Snapshot.cat([s.select(idx), s.cpu(), s.select(mask)])
    assert not both.is_host and np.array_equal(both.numpy(), np.concatenate([r[idx], r, r[mask]]))
    assert Snapshot.cat([s.cpu(), s]).is_host
    other = _vec(S, traceback=False)
    with pytest.raises(ValueError, match="traceback"):
        Snapshot.cat([s, Snapshot(torch.zeros((1, other.core.snapshot_info().record_bytes), dtype=torch.uint8),
                                  other.core.snapshot_info())])
    with pytest.raises(ValueError):
        Snapshot.cat([])
