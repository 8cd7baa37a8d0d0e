"""The guards of tests/test_gpu_counters64.py as tests of their own, without a GPU: on the oracle's
side alone, each 32-bit mistake in the counters of the counter-based RNG (the seed's upper half
dropped, ``env_offset + i`` or ``t0 + t`` wrapped to 32 bits, a playout id cut or its carry lost)
changes the action table in every 64-env wave it can reach, and the oracle's reward codes and rule
bits with it.  The GPU tests compute their references behind the same guards; here a guard that went
blind shows before any GPU run."""
import pytest

pytest.importorskip("torch")

from test_gpu_counters64 import T, _guard_picks, _guard_table, _ref, _rules_ref  # noqa: E402


@pytest.mark.parametrize("n", [256, 272, 300])
def test_guard_each_32_bit_mistake_changes_the_oracle_table(n):
    assert _guard_table(n)


@pytest.mark.parametrize("name,tb,n,autoreset", [("7x7_full", True, 256, "next_step"), ("7x7_full", False, 256, "none"),
                                                 ("mixed_5_11", True, 300, "next_step")])
def test_guard_each_32_bit_mistake_changes_the_oracle_rewards(name, tb, n, autoreset):
    assert _ref(name, tb, n, autoreset)["rew"].shape == (T, n)


def test_guard_playout_draws_depend_on_the_upper_halves():
    assert _guard_picks()


def test_guard_rule_rollout_sees_each_32_bit_mistake():
    assert _rules_ref("A", 300)["bits"].shape == (T, 300)
