"""CPU, no device library: the host logic of FusedAdam.set_visibility (visible-only Adam; fused_adam.py). The two launch functions of ops.py are replaced by recorders."""
import pytest
import torch


@pytest.fixture()
def calls(monkeypatch, lfs):
    from lichtfeld_studio_amd import ops
    log = []
    monkeypatch.setattr(ops, "adam_step_multi", lambda entries: log.append(("dense", list(entries))))
    monkeypatch.setattr(ops, "adam_step_multi_visible", lambda entries, bits, N: log.append(("visible", list(entries), bits, N)))
    monkeypatch.setattr(ops, "adam_step_wrapper", lambda *e: log.append(("single", e)))
    return log


def _optimizer(N=10, fused=True, extra=None):
    from lichtfeld_studio_amd.fused_adam import FusedAdam
    shapes = [(N, 3), (N, 1, 3), (N, 3, 3), (N, 3), (N, 4), (N,)]
    params = [torch.zeros(s, requires_grad=True) for s in shapes] + ([extra] if extra is not None else [])
    for p in params:
        p.grad = torch.ones_like(p)
    groups = [{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(params)]
    return FusedAdam(groups, fused=fused), params


def test_set_visibility_is_consumed_by_one_step(calls):
    opt, params = _optimizer()
    bits = torch.zeros(1, dtype=torch.int32)
    opt.set_visibility(bits, 10)
    opt.step(2000)
    opt.step(2001)
    assert [c[0] for c in calls] == ["visible", "dense"]
    kind, entries, got_bits, N = calls[0]
    assert got_bits is bits and N == 10 and len(entries) == 6
    assert all(e[0] is p for e, p in zip(entries, params))
    assert [opt.state[id(p)]["step_count"] for p in params] == [2] * 6
    # the scalars of the visible step are those of a dense first step: the bias corrections come from the global step count
    assert entries[0][8] == pytest.approx(1.0 / (1.0 - 0.9)) and calls[1][1][0][8] == pytest.approx(1.0 / (1.0 - 0.9 ** 2))


def test_a_parameter_without_n_rows_raises_and_the_visibility_is_still_consumed(calls):
    opt, _ = _optimizer(extra=torch.zeros(7, 2, requires_grad=True))
    opt.set_visibility(torch.zeros(1, dtype=torch.int32), 10)
    with pytest.raises(ValueError, match="N rows"):
        opt.step(2000)
    assert calls == []
    opt.step(2001)
    assert [c[0] for c in calls] == ["dense"]


def test_unfused_optimizer_refuses(calls):
    opt, _ = _optimizer(fused=False)
    with pytest.raises(ValueError, match="fused=True"):
        opt.set_visibility(torch.zeros(1, dtype=torch.int32), 10)
    opt.step(2000)
    assert [c[0] for c in calls] == ["single"] * 6


def test_the_shN_skip_still_advances_its_step_count(calls):
    opt, params = _optimizer()
    opt.set_visibility(torch.zeros(1, dtype=torch.int32), 10)
    opt.step(1000)                     # iteration <= 1000: group 3 (shN) is left out of the launch
    kind, entries, _, _ = calls[0]
    assert kind == "visible" and len(entries) == 5 and all(e[0] is not params[2] for e in entries)
    assert [opt.state[id(p)]["step_count"] for p in params] == [1] * 6
    opt.set_visibility(torch.zeros(1, dtype=torch.int32), 10)
    opt.step(1001)
    entries = calls[1][1]
    assert len(entries) == 6 and entries[2][0] is params[2]
    assert entries[2][8] == pytest.approx(1.0 / (1.0 - 0.9 ** 2))   # shN's second step by count, although its first update
