"""The contract between a model's backward and the gradient reducer attached to the module (dp.py), for all three models:
one begin() before the first announcement, every parameter announced exactly once and only when its gradient is final, in
backward order, finish() after the last one -- and _abort() instead of finish() when the backward raises, with the zero pool
closed either way.  The three training paths run the same block / decoder / stem / node code (blocks_train.py), so this is the
behaviour that code has to keep for each of them.

A recording stand-in takes the reducer's place (no process group, no all-reduce): a plain object with the four methods the
node calls.  Shapes: the smallest each model trains at by more than one route (FastTransformer 64 x 64 at x2: merged
patch_embed gradient, composed branch A; WindowTransformer 2 x 88 x 120; ResidualTransformer's token count is fixed by
pos_embed, so 720p it is)."""
import importlib
import re

import pytest
import torch

from transformerupscaler_amd import ops
from transformerupscaler_amd.autograd import l1_loss
from transformerupscaler_amd.dp import _ft_backward_key
from transformerupscaler_amd.weights import deterministic_state_dict, rt_deterministic_state_dict, wt_deterministic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = {          # plugin, state dict, strict, constructor keywords, LR shape, HR size
    "ft": ("FastTransformer", deterministic_state_dict, False, {}, (1, 3, 64, 64), (128, 128)),
    "wt": ("WindowTransformer", wt_deterministic_state_dict, False, {"dropout": 0.1}, (2, 3, 88, 120), (176, 240)),
    "rt": ("ResidualTransformer", rt_deterministic_state_dict, True, {}, (1, 3, 720, 1280), (4320, 7680)),
}


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.deterministic = False
    ops.release_det_slabs()


@pytest.fixture(scope="module")
def setups():
    """name -> (module, lr, hr), built on first use; no test here moves a weight."""
    made = {}

    def get(name):
        if name not in made:
            plugin, sd_fn, strict, kw, lr_shape, hr_hw = CASES[name]
            m = importlib.import_module(f"models.{plugin}.model").TransformerModel(**kw)
            m.load_state_dict(sd_fn(0), strict=strict)
            g = torch.Generator().manual_seed(77)
            made[name] = (m.to(DEV), torch.rand(lr_shape, generator=g).to(DEV), torch.rand((lr_shape[0], 3) + hr_hw, generator=g).to(DEV))
        return made[name]
    yield get
    made.clear()
    torch.cuda.empty_cache()


class Recorder:
    """Stands in for dp.GradReducer on module._grad_reducer; finish() hands back the backward's own gradient dict."""

    def __init__(self):
        self.events, self.g = [], None

    def begin(self, names):
        self.events.append(("begin", list(names)))

    def on_ready(self, names, g):
        self.g = g
        self.events.append(("ready", list(names), {n: tuple(g[n].shape) if n in g else None for n in names}))

    def finish(self):
        self.events.append(("finish",))
        return self.g

    def _abort(self):
        self.events.append(("abort",))


def _backward(m, lr, hr, reducer=None):
    """One forward + backward of the training step's loss (harness.train_step without the optimizer), same dropout masks every
    call.  Returns {parameter name: gradient}."""
    m.zero_grad(set_to_none=True)
    m._dropout_calls = 0
    m._grad_reducer = reducer
    try:
        out = m(lr, res_out=tuple(hr.shape[2:]), require_ratio=False)
        l1_loss(out, hr, fuse_into_model_backward=True).backward()
    finally:
        m._grad_reducer = None
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _stage_rank(name, nblocks):
    """Backward stage of a ResidualTransformer / WindowTransformer parameter."""
    head = {"decoder_conv2": 0, "decoder_conv1": 1, "patch_unembed": 2, "pos_embed": 3 + nblocks, "patch_embed": 3 + nblocks,
            "downsample": 4 + nblocks, "conv2": 5 + nblocks, "conv1": 5 + nblocks}
    blk = re.match(r"(?:window|transformer)_blocks\.(\d+)\.", name)
    return 3 + (nblocks - 1 - int(blk.group(1))) if blk else head[name.split(".")[0]]


def _check_protocol(name, m, rec):
    kinds = [e[0] for e in rec.events]
    params = {k: tuple(p.shape) for k, p in m.named_parameters()}
    # (a) one begin, first; one finish, last
    assert kinds[0] == "begin" and kinds[-1] == "finish" and set(kinds[1:-1]) == {"ready"}, kinds
    ready = [e for e in rec.events if e[0] == "ready"]
    announced = [n for e in ready for n in e[1]]
    # (b) what begin was told = what is announced, each once
    assert sorted(announced) == sorted(rec.events[0][1]) and len(set(announced)) == len(announced)
    # (c) announced = already in g, with the parameter's shape
    for e in ready:
        for n in e[1]:
            assert e[2][n] == params[n], (n, e[2][n], params[n])
    # (d) backward order
    if name == "ft":
        keys = [_ft_backward_key(n) for n in announced]
        assert keys == sorted(keys), keys
    else:
        nblocks = len(m.window_blocks if name == "wt" else m.transformer_blocks)
        ranks = [sorted({_stage_rank(n, nblocks) for n in e[1]}) for e in ready]
        assert ranks == [[r] for r in range(6 + nblocks)], ranks
        assert ("pos_embed" in announced) == (name == "rt")


@pytest.mark.parametrize("dropout", [True, False], ids=["dropout", "eval"])
@pytest.mark.parametrize("name", list(CASES))
def test_backward_announces_every_gradient_once_in_order(setups, name, dropout):
    m, lr, hr = setups(name)
    m.train(dropout)
    assert m.dropout_p > 0
    rec = Recorder()
    got = _backward(m, lr, hr, rec)          # the default route (atomic weight gradients, composed branch A, merged patch_embed)
    _check_protocol(name, m, rec)
    assert set(got) == set(rec.events[0][1])
    with ops.deterministic_mode():
        plain = _backward(m, lr, hr)
        rec = Recorder()
        got = _backward(m, lr, hr, rec)
    _check_protocol(name, m, rec)
    # (e) through the stand-in = without a reducer, bit for bit
    assert got.keys() == plain.keys() and len(got) == len(rec.events[0][1])
    differing = [k for k in got if not torch.equal(got[k], plain[k])]
    assert not differing, differing[:8]
    assert all(torch.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("name", ["ft", "wt"])
def test_a_failing_backward_aborts_the_episode_and_closes_the_zero_pool(setups, name, monkeypatch):
    m, lr, hr = setups(name)
    m.train()

    def boom(*a, **kw):
        raise RuntimeError("injected failure in conv1's weight gradient")
    rec = Recorder()
    with monkeypatch.context() as mp:
        mp.setattr(ops, "conv1_wgrad", boom)          # the last weight gradient of every model's backward
        with pytest.raises(RuntimeError, match="injected failure"):
            _backward(m, lr, hr, rec)
    kinds = [e[0] for e in rec.events]
    assert kinds[0] == "begin" and kinds[-1] == "abort" and "finish" not in kinds, kinds
    assert ops._zero_pool is None
    rec = Recorder()
    got = _backward(m, lr, hr, rec)          # the next step is a normal one
    _check_protocol(name, m, rec)
    assert all(torch.isfinite(v).all() for v in got.values())
