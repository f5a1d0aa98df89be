"""The Adam step kernel (csrc/adam.hip: ogc_adam_step, the NaN rule and the update over a table of chunks) against a float64
truth on DECIDED inputs (tests/adam_cases.py): every element of every output moves by at least 64 gate floors in one step, so a
skipped, doubled or misrouted element cannot pass.  The entry point is called through _lib.call on hand-built tables (the helper
DeviceState builds the pointer table, the chunk rows and the gradient pointer array as train_step._adam_kernel_step does); every
tensor sits in a buffer of its own between guard floats, which must keep their bits.

Tolerance, per output tensor of every case (test_group_norm_truth_gpu.Table).  The yardstick is torch.optim.Adam(foreach=False) in
fp32 on the host with the state injected, measured against the same float64 truth:
    err_kernel <= max(4 * err_torch32, 8 * 2**-24 * max|truth|)
for the max-abs error, and for the 2-norm of the error with the floor taken per element.  Both errors are printed per tensor (for
a case of more than 8 tensors: one line over all of them, and a line for every tensor that fails); nothing measured is written
into this file.  The step counts must equal step0 + 1 exactly, the flag must be 0.

On the CPU (unmarked): the float64 formula against torch's float64 Adam; the decided-input condition re-derived by that route; a
numpy mirror of the kernel's expressions and rounding points inside the gate on every case; seven wrong formulas outside it, with
the hyper-parameter sets that catch each; the branches the case list claims, re-derived from its chunk rows.

Relations on the GPU, bit for bit: a tensor against the same data split into several tensors with its step count (the update is
elementwise); a captured and replayed call against the eager one; a call refused or skipped by the NaN rule against the state
before it.  Out of scope: bf16 / fp64 parameters, amsgrad, tensors beyond 2**31 elements, a flag that is non-zero on entry.
"""
import contextlib
import copy
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import adam_cases as ac
from test_group_norm_truth_gpu import Table as _Table

gpu = pytest.mark.gpu
DEV = "cuda"
IDS = [ac.case_id(c) for c in ac.CASES]
C, T = ac.CHUNK, ac.THREADS


class Table(_Table):
    def __init__(self, name):
        self.name, self.bad = name, []


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.detach().cpu()


@functools.lru_cache(maxsize=None)
def yardstick(c, n_steps=1):
    """torch's fp32 Adam on the host, once per case; shared, never written to."""
    d = ac.make(c)
    return ac.torch_adam(d, d["hyper"], torch.float32, n_steps)


def check_state(tab, got, tr, yard, skip=()):
    """The gate on every tensor of param, exp_avg and exp_avg_sq (all but the tensors in `skip`)."""
    n = len(tr["param"])
    for name in ac.NAMES:
        if n > 8:
            cat = lambda s: torch.cat([_t(a).double().reshape(-1) for i, a in enumerate(s[name]) if i not in skip])  # noqa: E731
            tab.check("%s[all %d]" % (name, n - len(skip)), cat(got), cat(tr), cat(yard))
        for i in range(n):
            if i in skip:
                continue
            out = io.StringIO()
            with contextlib.redirect_stdout(out):
                tab.check("%s[%d]" % (name, i), _t(got[name][i]), _t(tr[name][i]), _t(yard[name][i]))
            if n <= 8 or "FAILS" in out.getvalue():
                print(out.getvalue(), end="")


# ---- the generator's guarantees, the truth, the gate's power (CPU) -----------------------------------------------------------------------
@pytest.mark.parametrize("h", range(len(ac.HYPERS)))
def test_truth_is_torch_float64_adam(h):
    """adam_cases.truth against torch.optim.Adam on float64 CPU tensors (an independent route to the same numbers), one step and
    two, to 1e-14 relative."""
    d = ac.make(ac.MIXED_CASES[h])
    for n_steps in (1, 2):
        tr, ref = ac.truth(d, d["hyper"], n_steps), ac.torch_adam(d, d["hyper"], torch.float64, n_steps)
        assert tr["step"] == ref["step"] == [s + n_steps for s in d["step"]]
        for name in ac.NAMES:
            for i, (got, want) in enumerate(zip(tr[name], ref[name])):
                want = want.numpy()
                assert want.dtype == np.float64 and got.dtype == np.float64
                assert float(np.abs(got - want).max()) <= 1e-14 * float(np.abs(want).max()), (h, n_steps, name, i)


@pytest.mark.parametrize("c", ac.CASES, ids=IDS)
def test_case_is_decided(c):
    """Re-checks what adam_cases.make asserts, with torch's float64 Adam as the truth: the input ranges, distinct tensors with
    their own step counts, and that EVERY element of all three outputs moves by at least 64 gate floors."""
    d = ac.make(c)
    h = d["hyper"]
    ref = ac.torch_adam(d, h, torch.float64)
    assert d["step"] == [h.step0 + i % 3 for i in range(len(c.sizes))]
    assert [a.size for a in d["param"]] == list(c.sizes)
    seen = set()
    for i, n in enumerate(c.sizes):
        p, g, m, v = (d[k][i] for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
        assert np.abs(p).min() >= 0.5 and np.abs(p).max() <= 1.5 and np.abs(g).min() >= np.float32(0.1) and np.abs(g).max() <= 1
        if h.step0 == 0:
            assert not m.any() and not v.any()
        else:
            assert np.abs(m).min() >= np.float32(0.05) and np.abs(m).max() <= 0.5 and bool((m * g > 0).all())
            assert v.min() >= np.float32(0.01) and v.max() <= 0.5
        seen.add((p[0].item(), g[0].item()))
    assert len(seen) == len(c.sizes)                                 # every tensor has values of its own
    worst = {}
    for name in ac.NAMES:
        worst[name] = min(float(np.abs(t.numpy() - a.astype(np.float64)).min()) / (8 * ac.U * float(t.abs().max()))
                          for a, t in zip(d[name], ref[name]))
        assert worst[name] >= ac.DECIDED, (name, worst[name])
        assert abs(worst[name] - d["margin"][name]) <= 1e-6 * worst[name]
    print("%-16s least move in gate floors: param %.0f  exp_avg %.0f  exp_avg_sq %.0f"
          % (ac.case_id(c), worst["param"], worst["exp_avg"], worst["exp_avg_sq"]))


@pytest.mark.parametrize("c", ac.CASES, ids=IDS)
def test_mirror_passes_the_gate(c):
    """The kernel's expressions with its rounding points, in numpy: inside the gate on every case, so the gate asks nothing of
    the kernel that its documented arithmetic cannot give."""
    d = ac.make(c)
    tab = Table(ac.case_id(c) + " mirror")
    got = ac.mirror(d, d["hyper"])
    assert all(a.dtype == np.float32 for name in ac.NAMES for a in got[name]) and got["step"] == d["truth"]["step"]
    check_state(tab, got, d["truth"], yardstick(c))
    tab.done()


# mutant: (sets that MUST catch it, sets that cannot) — indices into adam_cases.HYPERS, on the `mixed` layout.  A set in neither
# is within a small factor of the gate (it depends on the yardstick's own rounding); it is printed and not asserted.
#   step_not_plus_one  the corrections of the step before: 1 - beta**0 = 0 at set 0 (a division by zero), far off at steps 1..7
#                      (sets 1, 3); at 100000 both are 1 either way; at step 999 only bc2 moves, by 6e-4 relative: half a floor
#   no_weight_decay    exp_avg moves by (1 - beta1) * weight_decay * |param| >= 5e-6, twenty floors; set 2 has no decay to lose
#   sq_before_decay    exp_avg_sq moves by (1 - beta2) * 2 * weight_decay * |grad * param|: 3e-3 at set 3, up to 3e-7 at
#                      beta2 = 0.999, where a floor of exp_avg_sq is 2.4e-7 (sets 1, 4: marginal) but 5e-10 on a first step (set 0)
#   decoupled_decay    as no_weight_decay, in exp_avg
#   bc2_not_rooted     bc2 against its root: 0.632 against 0.795 at step 999, further apart before, both 1 at set 4
#   eps_in_root        sqrt(v / bc2 + eps) against sqrt(v / bc2) + eps: at 1e-8 the parameter moves by 1e-8 of its update, 1e-3 shows
#   eps_over_bc2       eps / sqrt(bc2): as little at 1e-8; at 1e-3 the denominator moves by 5 % (set 1) and 0.1 % (set 3)
CAUGHT_ON = {
    "step_not_plus_one": ({0, 1, 3}, {4}),
    "no_weight_decay": ({0, 1, 3, 4}, {2}),
    "sq_before_decay": ({0, 3}, {2}),
    "decoupled_decay": ({0, 1, 3, 4}, {2}),
    "bc2_not_rooted": ({0, 1, 2, 3}, {4}),
    "eps_in_root": ({1, 3}, {0, 2, 4}),
    "eps_over_bc2": ({1, 3}, {0, 2, 4}),
}


@pytest.mark.parametrize("mutant", ac.MUTANTS)
def test_mutants_fail_the_gate(mutant):
    """Each wrong formula, evaluated in float64 (so nothing but the mistake separates it from the truth), fails the gate on the
    sets CAUGHT_ON says it must, and passes where the mistake cannot show; set 3 catches all seven."""
    caught = set()
    for c in ac.MIXED_CASES:
        d = ac.make(c)
        tab = Table("%s %s" % (ac.case_id(c), mutant))
        with contextlib.redirect_stdout(io.StringIO()):
            check_state(tab, ac.mutated(d, d["hyper"], mutant), d["truth"], yardstick(c))
        if tab.bad:
            caught.add(c.hyper)
        print("%-24s set %d: %s" % (mutant, c.hyper, "fails in %d of %d tensors" % (len(tab.bad), 3 * len(c.sizes)) if tab.bad
                                    else "passes"))
    must, never = CAUGHT_ON[mutant]
    assert 3 in must and must <= caught and not (never & caught), (mutant, caught)


def test_case_list_reaches_its_branches():
    """The (tensor, offset) rows of every case, built by the expression of _adam_kernel_step, replayed: every property the case
    list's comments name is there."""
    assert ac.rows((5,)) == [(0, 0)] and ac.rows((C, C + 1)) == [(0, 0), (1, 0), (1, C)]
    singles = sorted({c.sizes[0] for c in ac.CASES if len(c.sizes) == 1})
    assert singles == [1, T - 1, T, T + 1, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 1]
    assert [len(ac.rows((n,))) for n in singles] == [1, 1, 1, 1, 1, 1, 2, 2, 3, 4]
    last = [n - ac.rows((n,))[-1][1] for n in singles]                       # elements of the last chunk
    assert last == [1, T - 1, T, T + 1, C - 1, C, 1, C, 1, 1] and C % T == 0 and (C - 1) % T == T - 1
    by_name = {}
    for c in ac.CASES:
        by_name.setdefault(c.name, []).append(c)
        assert sum(c.sizes) <= 10 ** 5 and len(c.sizes) <= ac.MAX_TENSORS and min(c.sizes) >= 1
        assert all(0 <= off < c.sizes[i] and off % C == 0 for i, off in ac.rows(c.sizes))
    assert all(len({c.hyper for c in cs}) >= 2 for cs in by_name.values())   # every layout under two sets at least
    assert {c.hyper for c in ac.CASES if len(c.sizes) == 1} == set(range(len(ac.HYPERS)))
    assert [c.hyper for c in ac.MIXED_CASES] == list(range(len(ac.HYPERS)))
    assert [c for c in ac.CASES if c.offset] == [ac.case("mixed", ac.MIXED, 1, offset=1)]
    # mixed
    assert ac.MIXED == (1, 4097, 3, 2048, 2049, 7, 6145, 1) or C != 2048
    r = ac.rows(ac.MIXED)
    multi = [i for i, n in enumerate(ac.MIXED) if n > C]
    assert multi == [1, 4, 6] and all(ac.MIXED[i - 1] == 1 or ac.MIXED[i + 1] == 1 for i in (1, 6))
    follows = [(a, b) for a, b in zip(r, r[1:]) if a[1] != 0 and b[1] == 0]       # an off != 0 row next to the next tensor's first
    assert len(follows) == 3 and all(b[0] == a[0] + 1 for a, b in follows)
    assert [ac.MIXED[i] - max(off for t, off in r if t == i) for i in multi] == [1, 1, 1]     # ragged last chunks
    assert len(r) == 1 + 3 + 1 + 1 + 2 + 1 + 4 + 1
    # many: 105 tensors, large and tiny alternating
    assert len(ac.MANY) == 105 > 6 and set(ac.MANY) == {1, 13, 300, C + 1}
    r = ac.rows(ac.MANY)
    assert sum(1 for a, b in zip(r, r[1:]) if a[1] != 0 and b[1] == 0 and ac.MANY[b[0]] == 1) >= 26
    # limit
    assert len(ac.LIMIT) == ac.MAX_TENSORS and set(ac.LIMIT) == {1, 2, 3, 4, 5} and len(ac.rows(ac.LIMIT)) == ac.MAX_TENSORS
    # the hyper-parameter sets
    hs = ac.HYPERS
    assert [h.step0 for h in hs] == [0, 1, 999, 5, 100000] and [h.weight_decay for h in hs] == [1e-4, 1e-4, 0.0, 1e-2, 1e-4]
    assert np.float32(1 - 0.9 ** 100001) == 1 and np.float32(1 - 0.999 ** 100001) == 1
    assert ac.GUARD == 8 and np.isnan(np.array([ac.GUARD_BITS], np.int32).view(np.float32)[0])


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import ogc_amd  # noqa: F401  (fails loudly if libogc_ops.so is missing)
    from ogc_amd import _lib
    L = _lib.load()
    assert L.ogc_adam_chunk() == C and L.ogc_adam_max_tensors() == ac.MAX_TENSORS     # what adam_cases read from the source
    return _lib


def _guarded(a, offset):
    """(buffer, view): `a` on the device, GUARD + offset guard floats before it and GUARD after it."""
    n, lead = a.size, ac.GUARD + offset
    buf = torch.empty(lead + n + ac.GUARD, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(ac.GUARD_BITS)
    view = buf[lead:lead + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return buf, view


class DeviceState:
    """The tensors of a state (adam_cases.make, or any dict with its keys) on the device, each in a guarded buffer of its own, with
    the table, the chunk rows, the snapshot and the flag of ogc_adam_step."""
    KINDS = ac.NAMES + ("grad",)

    def __init__(self, state, offset=0):
        self.sizes = [a.size for a in state["param"]]
        self.n, self.offset = len(self.sizes), offset
        self.buf, self.view = {k: [] for k in self.KINDS}, {k: [] for k in self.KINDS}
        for k in self.KINDS:
            for a in state[k]:
                b, v = _guarded(a, offset)
                self.buf[k].append(b), self.view[k].append(v)
        self.step_buf, self.steps = _guarded(np.asarray(state["step"], np.float32), 0)
        table = [[v.data_ptr() for v in self.view[k]] for k in ac.NAMES]
        table += [[self.steps[i:].data_ptr() for i in range(self.n)], self.sizes]
        self.pieces = ac.rows(self.sizes)
        self.table = torch.tensor(table, dtype=torch.int64, device=DEV)
        self.chunks = torch.tensor(self.pieces, dtype=torch.int32, device=DEV)
        self.snapshot = torch.zeros(self.n, dtype=torch.float32, device=DEV)
        self.flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def grad_array(self):
        return (ctypes.c_void_p * self.n)(*[v.data_ptr() for v in self.view["grad"]])

    def call(self, lib, h, n_tensors=None, n_chunks=None, table=True, grads=...):
        lib.call("ogc_adam_step", self.n if n_tensors is None else n_tensors, len(self.pieces) if n_chunks is None else n_chunks,
                 self.table.data_ptr() if table else None, self.chunks.data_ptr(), self.grad_array() if grads is ... else grads,
                 self.snapshot.data_ptr(), self.flag.data_ptr(), h.lr, h.beta1, h.beta2, h.eps, h.weight_decay,
                 torch.cuda.current_stream().cuda_stream)

    def bits(self):
        """Every buffer the call may write (parameters, moments, step counts — guards included), as int32 copies."""
        return [b.view(torch.int32).clone() for k in ac.NAMES for b in self.buf[k]] + [self.step_buf.view(torch.int32).clone()]

    def same_bits(self, before):
        return all(torch.equal(a, b) for a, b in zip(self.bits(), before))

    def guards_intact(self):
        lead = ac.GUARD + self.offset
        for k in self.KINDS:
            for b, n in zip(self.buf[k], self.sizes):
                g = b.view(torch.int32)
                if not (bool((g[:lead] == ac.GUARD_BITS).all()) and bool((g[lead + n:] == ac.GUARD_BITS).all())):
                    return False
        g = self.step_buf.view(torch.int32)
        return bool((g[:ac.GUARD] == ac.GUARD_BITS).all()) and bool((g[ac.GUARD + self.n:] == ac.GUARD_BITS).all())

    def got(self):
        out = {k: [v.cpu() for v in self.view[k]] for k in ac.NAMES}
        out["step"] = self.steps.cpu().tolist()
        return out


def _settled(dev, steps, flag=0):
    """The flag, the step counts (exactly) and the guards after a call."""
    assert int(dev.flag.item()) == flag
    assert dev.steps.cpu().tolist() == [float(s) for s in steps]
    assert dev.guards_intact()


# ---- truth ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", ac.CASES, ids=IDS)
def test_truth(lib, c):
    """One call against the float64 truth of one step, a second call on the same tables against the truth of two; the step counts
    advance by exactly one per call in every tensor (once, not once per chunk), the flag stays 0, the guards keep their bits."""
    d = ac.make(c)
    h = d["hyper"]
    dev = DeviceState(d, c.offset)
    assert all((v.data_ptr() % 16 != 0) == bool(c.offset) for k in dev.KINDS for v in dev.view[k])
    dev.call(lib, h)
    _settled(dev, d["truth"]["step"])
    tab = Table(ac.case_id(c))
    check_state(tab, dev.got(), d["truth"], yardstick(c))
    dev.call(lib, h)
    _settled(dev, [s + 2 for s in d["step"]])
    tab.name += " x2"
    check_state(tab, dev.got(), ac.truth(d, h, 2), yardstick(c, 2))
    tab.done()


@gpu
def test_split_tensor_gives_the_same_bits(lib):
    """The update is elementwise: a tensor of 3 chunks + 1 and the same data cut into tensors that share its step count (cuts
    inside a chunk, at a chunk's edge and one element from the end) give identical bits in all three outputs."""
    c = ac.case("single%d" % (3 * C + 1), (3 * C + 1,), 3)
    assert c in ac.CASES
    d = ac.make(c)
    cuts = [0, 1, T + 3, C, 2 * C + 5, 3 * C, 3 * C + 1]
    parts = {k: [d[k][0][a:b] for a, b in zip(cuts, cuts[1:])] for k in DeviceState.KINDS}
    parts["step"] = [d["step"][0]] * (len(cuts) - 1)
    whole, split = DeviceState(d), DeviceState(parts)
    assert len(split.pieces) > len(whole.pieces)
    whole.call(lib, d["hyper"]), split.call(lib, d["hyper"])
    _settled(whole, d["truth"]["step"]), _settled(split, [d["step"][0] + 1] * split.n)
    for k in ac.NAMES:
        assert torch.equal(torch.cat(split.view[k]).view(torch.int32), whole.view[k][0].view(torch.int32)), k


@gpu
def test_captured_call_leaves_the_eager_bits(lib):
    """The call captured once in a HIP graph (the flag zeroed inside the capture) and replayed, against the eager call."""
    c = ac.MIXED_CASES[1]
    d = ac.make(c)
    eager, replayed = DeviceState(d), DeviceState(d)
    eager.call(lib, d["hyper"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.flag.zero_()
        replayed.call(lib, d["hyper"])
    graph.replay()
    torch.cuda.synchronize()
    _settled(eager, d["truth"]["step"]), _settled(replayed, d["truth"]["step"])
    assert replayed.same_bits(eager.bits())


# ---- the NaN rule -------------------------------------------------------------------------------------------------------------------------
QUIET_NAN, NEGATIVE_NAN, PAYLOAD_NAN = 0x7FC00000, 0xFFC00000 - 2 ** 32, 0x7F800001
# (tensor of `mixed`, element, bit pattern): every place a NaN is put, one at a time
NAN_PLACES = [
    (0, 0, QUIET_NAN),                          # element 0 of tensor 0
    (6, 3 * C, QUIET_NAN),                      # the last element of the ragged last chunk of the last multi-chunk tensor
    (1, C + 5, QUIET_NAN),                      # an element of an off != 0 chunk
    (6, C + 63, QUIET_NAN),                     # the last lane of a workgroup's first wave
    (6, C + 64, QUIET_NAN),                     # the first lane of its second
    (6, C + 255, QUIET_NAN),                    # its last thread
    (3, 3 * T + 64, QUIET_NAN),                 # the same lane in a later stride
    (7, 0, QUIET_NAN),                          # the only element of a one-element tensor (the last row of the table)
    (4, C, NEGATIVE_NAN),                       # a negative NaN
    (2, 1, PAYLOAD_NAN),                        # a NaN with a non-default payload (signalling)
]


@gpu
def test_nan_rule_skips_everything(lib):
    """One NaN in a gradient, wherever it sits: the flag is 1 and every parameter, moment, step count and guard keeps its bits.
    With the NaN taken out again the same tables step as usual."""
    c = ac.MIXED_CASES[3]
    d = ac.make(c)
    h = d["hyper"]
    dev = DeviceState(d)
    before = dev.bits()
    assert max(i for i, n in enumerate(ac.MIXED) if n > C) == 6 and ac.MIXED[6] == 3 * C + 1 and ac.MIXED[7] == 1
    for ti, e, pattern in NAN_PLACES:
        assert 0 <= e < ac.MIXED[ti]
        g = dev.view["grad"][ti].view(torch.int32)
        keep = int(g[e].item())
        g[e] = pattern
        assert bool(torch.isnan(dev.view["grad"][ti][e]))
        dev.flag.zero_()
        dev.call(lib, h)
        _settled(dev, d["step"], flag=1)
        assert dev.same_bits(before), (ti, e)
        g[e] = keep
    dev.flag.zero_()
    dev.call(lib, h)
    _settled(dev, d["truth"]["step"])
    tab = Table(ac.case_id(c) + " after NaNs")
    check_state(tab, dev.got(), d["truth"], yardstick(c))
    tab.done()


def _poisoned(c, kind, ti, e, value):
    """The state of case c with one element replaced, and its float64 truth and host yardstick."""
    d = ac.make(c)
    state = {k: list(d[k]) for k in DeviceState.KINDS + ("step",)}
    state[kind][ti] = d[kind][ti].copy()
    state[kind][ti][e] = value
    with np.errstate(all="ignore"):
        return state, ac.truth(state, d["hyper"]), ac.torch_adam(state, d["hyper"])


@gpu
@pytest.mark.parametrize("kind, value", [("param", np.nan), ("exp_avg", np.nan), ("exp_avg_sq", np.nan), ("grad", np.inf)])
def test_rule_fires_on_gradient_nans_only(lib, kind, value):
    """A NaN in a parameter or a moment and none in a gradient, or a +inf gradient element (not a NaN): the flag stays 0 and the
    step counts advance, as torch's rule (_foreach_norm, sum, isnan) has it.  Every other tensor meets the gate; in the poisoned
    one the non-finite elements are those of the host yardstick, and the finite ones meet the gate."""
    c = ac.MIXED_CASES[1]                        # (beta1 = 0.9: at 0.5 torch's lerp_ turns an infinite gradient into inf - inf)
    d = ac.make(c)
    ti, e = 4, C                                 # the one-element ragged chunk of a two-chunk tensor
    state, tr, yard = _poisoned(c, kind, ti, e, value)
    norms = torch._foreach_norm([torch.from_numpy(g) for g in state["grad"]])
    assert not bool(torch.isnan(torch.stack(norms).sum()))                     # torch's rule does not fire either
    dev = DeviceState(state)
    dev.call(lib, d["hyper"])
    _settled(dev, tr["step"])
    got = dev.got()
    tab = Table("%s %s[%d][%d]=%s" % (ac.case_id(c), kind, ti, e, value))
    check_state(tab, got, tr, yard, skip={ti})
    finite = np.ones(ac.MIXED[ti], bool)
    finite[e] = False
    for name in ac.NAMES:
        g, y, t = got[name][ti].numpy(), yard[name][ti].numpy(), tr[name][ti]
        assert np.array_equal(np.isnan(g), np.isnan(y)) and np.array_equal(np.isnan(g), np.isnan(t)), name
        assert np.array_equal(g[np.isinf(g)], y[np.isinf(y)]) and np.array_equal(np.isinf(g), np.isinf(t)), name
        assert np.isfinite(g[finite]).all() and (kind == "grad" or name != kind or not np.isfinite(g[e]))
        tab.check("%s[%d] finite" % (name, ti), _t(g[finite]), _t(t[finite]), _t(y[finite]))
    assert not np.isfinite(got["param"][ti].numpy()[e])                        # the poison does reach the parameter
    tab.done()


# ---- refusals of the C entry point ----------------------------------------------------------------------------------------------------------
@gpu
def test_entry_point_refusals(lib):
    """Well-formed arguments that ogc_adam_step is documented to refuse: an error return with a message, nothing launched (no
    output changes, the flag stays 0); empty calls return OK and touch nothing."""
    c = ac.MIXED_CASES[1]
    d = ac.make(c)
    h = d["hyper"]
    dev = DeviceState(d)
    before = dev.bits()
    too_many = ac.MAX_TENSORS + 1
    some = dev.view["grad"][0].data_ptr()
    with_null = dev.grad_array()
    with_null[3] = None
    refused = [
        (dict(n_tensors=too_many, n_chunks=1, grads=(ctypes.c_void_p * too_many)(*[some] * too_many)), "more than %d tensors" % ac.MAX_TENSORS),
        (dict(grads=with_null), "null gradient pointer"),
        (dict(table=False), "null pointer"),
        (dict(grads=None), "null pointer"),
        (dict(n_tensors=-1), "negative size"),
        (dict(n_chunks=-1), "negative size"),
    ]
    for kwargs, message in refused:
        with pytest.raises(lib.OgcOpsError, match=message):
            dev.call(lib, h, **kwargs)
        assert int(dev.flag.item()) == 0 and dev.same_bits(before), kwargs
    for kwargs in (dict(n_tensors=0), dict(n_chunks=0), dict(n_tensors=0, n_chunks=0)):
        dev.call(lib, h, **kwargs)
        assert int(dev.flag.item()) == 0 and dev.same_bits(before), kwargs
    dev.call(lib, h)                                                            # and the same object still steps
    _settled(dev, d["truth"]["step"])
    assert not dev.same_bits(before)


# ---- the Python path ------------------------------------------------------------------------------------------------------------------------
def _nets(empty=False):
    """Two identical nets: one weight of three chunks and more (70 x 96), small ones, optionally a parameter without elements."""
    torch.manual_seed(5)
    a = torch.nn.Sequential(torch.nn.Linear(96, 70), torch.nn.GroupNorm(1, 70), torch.nn.Linear(70, 5)).to(DEV)
    assert a[0].weight.numel() > 3 * C
    if empty:
        a.register_parameter("nothing", torch.nn.Parameter(torch.empty(0, device=DEV)))
    return a, copy.deepcopy(a)


def _backward(nets, x):
    for net in nets:
        net.zero_grad(set_to_none=True)
        net(x).square().sum().backward()
        if getattr(net, "nothing", None) is not None:
            net.nothing.grad = torch.empty(0, device=DEV)


def _step_counts(opt):
    return [float(opt.state[p]["step"]) for p in opt.param_groups[0]["params"]]


def _same_training(a, b, oa, ob, what):
    """Parameters and moments to fp32 rounding (the tolerances of test_fast_adam_gpu), step counts exactly."""
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, rtol=2e-6, atol=1e-7), (what, float((pa - pb).abs().max()))
        for name in ("exp_avg", "exp_avg_sq"):
            sa, sb = oa.state[pa][name], ob.state[pb][name]
            assert torch.allclose(sa, sb, rtol=1e-5, atol=2e-6), (what, name, float((sa - sb).abs().max()))
    assert _step_counts(oa) == _step_counts(ob), what


@gpu
def test_python_path_on_a_multi_chunk_net(lib):
    """train_step._adam_kernel_step against optimizer.step() of a twin on a net whose first weight spans four chunks; the tables
    are rebuilt when a parameter's storage is replaced (the old storage keeps its bits, the new one is stepped)."""
    from ogc_amd.train_step import _adam_kernel_step, make_optimizer
    a, b = _nets()
    oa, ob = make_optimizer(a.parameters(), 1e-2, weight_decay=1e-4), make_optimizer(b.parameters(), 1e-2, weight_decay=1e-4)
    used = []
    for step in range(5):
        _backward((a, b), torch.randn(4, 96, device=DEV))
        if step == 3:
            old = a[0].weight.data
            old_bits = old.view(torch.int32).clone()
            a[0].weight.data = old.clone()
            assert a[0].weight.data_ptr() != old.data_ptr()
        flag = _adam_kernel_step(oa)
        used.append(flag is not None)
        if flag is None:
            oa.step()
        else:
            assert int(flag.item()) == 0
        ob.step()
        _same_training(a, b, oa, ob, step)
        if step == 3:
            assert torch.equal(old.view(torch.int32), old_bits)                 # the stale pointer was not written through
            assert oa._ogc_adam_tables["ptrs"][0] == a[0].weight.data_ptr()
    assert used == [False, True, True, True, True], used      # the first step builds the state through torch
    assert _step_counts(oa) == [5.0] * 6


@gpu
def test_python_path_declines_what_it_does_not_cover(lib):
    """None (the caller then takes the torch path) for more than ogc_adam_max_tensors() parameters, for two parameter groups and
    for a non-contiguous gradient; the flag for the same optimizers inside the limits."""
    from ogc_amd.train_step import _adam_kernel_step, make_optimizer

    def ready(groups):
        opt = torch.optim.Adam(groups, lr=1e-2, fused=True) if isinstance(groups[0], dict) else make_optimizer(groups, 1e-2)
        for g in opt.param_groups:
            for p in g["params"]:
                p.grad = torch.ones_like(p)
        opt.step()                                                              # the state exists now
        return opt

    params = [torch.nn.Parameter(torch.full((2,), float(i + 1), device=DEV)) for i in range(ac.MAX_TENSORS + 1)]
    assert _adam_kernel_step(ready(params)) is None
    flag = _adam_kernel_step(ready(params[:-1]))
    assert flag is not None and int(flag.item()) == 0
    assert _adam_kernel_step(ready([{"params": params[:2]}, {"params": params[2:4]}])) is None
    w = torch.nn.Parameter(torch.ones(70, 96, device=DEV))
    opt = ready([w, params[0]])
    w.grad = torch.ones(96, 70, device=DEV).t()
    assert w.grad.shape == w.shape and not w.grad.is_contiguous()
    before = w.detach().clone()
    assert _adam_kernel_step(opt) is None and torch.equal(w, before)
    w.grad = w.grad.contiguous()
    flag = _adam_kernel_step(opt)
    assert flag is not None and int(flag.item()) == 0 and not torch.equal(w, before)


@gpu
def test_parameter_without_elements_keeps_its_step_count_in_line(lib):
    """A parameter with numel() == 0 has no chunk row, so the kernel could not move its step count, while optimizer.step() does;
    and its gradient's data_ptr() is null, which ogc_adam_step refuses (this test first met that refusal as an exception out of
    the training step).  _adam_kernel_step declines such an optimizer (None), and after every step, on whichever path, the
    parameters, moments and the counts of ALL parameters equal the twin's."""
    from ogc_amd.train_step import _adam_kernel_step, make_optimizer
    a, b = _nets(empty=True)
    oa, ob = make_optimizer(a.parameters(), 1e-2, weight_decay=1e-4), make_optimizer(b.parameters(), 1e-2, weight_decay=1e-4)
    assert len(oa.param_groups[0]["params"]) == 7
    for step in range(3):
        _backward((a, b), torch.randn(4, 96, device=DEV))
        flag = _adam_kernel_step(oa)
        if flag is None:
            oa.step()
        else:
            assert int(flag.item()) == 0
        ob.step()
        _same_training(a, b, oa, ob, step)
        assert _step_counts(oa) == [float(step + 1)] * 7
