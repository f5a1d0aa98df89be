"""Decided inputs and a float64 truth for the Adam step kernel (csrc/adam.hip: ogc_adam_step), for
tests/test_adam_truth_gpu.py.  Host side: numpy for the inputs and the truth, CPU torch for the yardstick; no GPU needed, the
library is not imported (CHUNK, THREADS and MAX_TENSORS are read from the kernel's source; the GPU tests hold them against
ogc_adam_chunk() / ogc_adam_max_tensors()).  The sibling of tests/bn_cases.py and tests/gn_cases.py.

Truth: adam64 — one Adam step from the definition, in float64, from the same fp32 inputs (test_truth_is_torch_float64_adam holds it
against torch.optim.Adam on float64 tensors).  Yardstick: torch.optim.Adam(foreach=False) in fp32 on the host, state injected.

"Decided" here means that a skipped, doubled or misrouted element can never hide inside the gate
    err_kernel <= max(4 * err_torch32, 8 * 2**-24 * max|truth|)            (test_group_norm_truth_gpu.Table)
because every element of every output moves by at least 64 gate floors in one step:
  * |param| uniform in [0.5, 1.5], random sign; |grad| uniform in [0.1, 1], random sign;
  * exp_avg has the sign of its gradient and magnitude in [0.05, 0.5]; exp_avg_sq lies in [0.01, 0.5]; elements whose moment
    would sit within MOMENT_GAP of the value the update pulls it towards (the decayed gradient, its square) are drawn again,
    inside the same ranges;
  * on a first-step case (step0 == 0) both moments are exactly zero;
  * every tensor of a case has its own values (the seed depends on the tensor's index) and its own step count
    (step0 + index % 3), so a chunk routed to a neighbouring tensor shows in all three outputs.
make() asserts  min |truth - input| >= 64 * 8 * 2**-24 * max|truth|  per tensor over ALL elements of param, exp_avg and
exp_avg_sq.  A case that misses it gets another seed or other ranges; the factor stays.

Out of scope: bf16 / fp64 parameters, amsgrad, tensors beyond 2**31 elements, a flag that is non-zero on entry.
"""
import collections
import functools
import math
import os
import re

import numpy as np
import torch

U = 2.0 ** -24
DECIDED = 64                    # every element moves by at least this many gate floors
GUARD = 8                       # floats of GUARD_BITS on either side of every tensor
GUARD_BITS = -3824219           # 0xFFC5A5A5 as int32: a negative NaN with a payload — a gradient read there trips the NaN rule
MOMENT_GAP = (0.01, 0.02)       # least |grad' - exp_avg| and |grad'^2 - exp_avg_sq| (grad' = grad + weight_decay * param)
NAMES = ("param", "exp_avg", "exp_avg_sq")


def _source_constant(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "ogc_amd", "csrc", "adam.hip")
    with open(path) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


THREADS = _source_constant("ADAM_THREADS")          # 256
CHUNK = _source_constant("ADAM_CHUNK")              # 2048
MAX_TENSORS = _source_constant("ADAM_MAX_TENSORS")  # 320

Hyper = collections.namedtuple("Hyper", "step0 lr beta1 beta2 eps weight_decay")
HYPERS = (
    Hyper(0, 1e-2, 0.9, 0.999, 1e-8, 1e-4),        # 0  first step: both moments zero, bias corrections at their smallest
    Hyper(1, 1e-2, 0.9, 0.999, 1e-3, 1e-4),        # 1  an eps that shows; sqrt(bc2) = 0.045..0.063, so its place shows too
    Hyper(999, 3e-3, 0.9, 0.999, 1e-8, 0.0),       # 2  weight_decay == 0: the other branch; a late step, another lr
    Hyper(5, 1e-2, 0.5, 0.9, 1e-3, 1e-2),          # 3  other betas, a weight decay and an eps that both show: every mutant fails here
    Hyper(100000, 1e-3, 0.9, 0.999, 1e-8, 1e-4),   # 4  both bias corrections are 1 in fp32
)

# sizes: elements of each tensor, in table order.  hyper: index into HYPERS.  offset: floats between the guard and the tensor's
# first element (1: the tensor is 4-byte aligned only).
Case = collections.namedtuple("Case", "name sizes hyper offset seed")


def case(name, sizes, hyper, offset=0, seed=0):
    return Case(name, tuple(sizes), hyper, offset, seed)


def case_id(c):
    return "%s-h%d" % (c.name, c.hyper) + ("-mis" if c.offset else "")


def single(n, *hypers):
    return [case("single%d" % n, (n,), h) for h in hypers]


MIXED = (1, 2 * CHUNK + 1, 3, CHUNK, CHUNK + 1, 7, 3 * CHUNK + 1, 1)
MANY = tuple((1, 13, 300, CHUNK + 1)[i % 4] for i in range(105))
LIMIT = tuple(1 + i % 5 for i in range(MAX_TENSORS))

CASES = (
    single(1, 0, 3)                                 # one element: one thread of one workgroup works
    + single(THREADS - 1, 1, 4)                     # one thread idle in the only stride
    + single(THREADS, 2, 3)                         # exactly one stride of the workgroup
    + single(THREADS + 1, 0, 3)                     # a second stride with one live thread
    + single(CHUNK - 1, 1, 4)                       # one element short of a full chunk: the last stride ragged by one
    + single(CHUNK, 2, 3)                           # a full chunk and no second one
    + single(CHUNK + 1, 0, 3)                       # two chunks (off != 0), the second holds one element
    + single(2 * CHUNK, 1, 4)                       # two full chunks
    + single(2 * CHUNK + 1, 2, 3)                   # two full chunks and a ragged third
    + single(3 * CHUNK + 1, 0, 3)                   # four chunks
    + [case("mixed", MIXED, h) for h in range(len(HYPERS))]   # multi-chunk tensors between one-element ones: off != 0 rows of one
                                                              # tensor next to off == 0 rows of the next; every hyper-parameter set
    + [case("mixed", MIXED, 1, offset=1)]           # every tensor one float into its buffer: 4-byte alignment only
    + [case("many", MANY, h) for h in (2, 3)]       # 105 tensors (segnet_kitti's count), chunk rows of large and tiny ones interleaved
    + [case("limit", LIMIT, h) for h in (0, 4)]     # exactly MAX_TENSORS tensors: the last gradient pointer of the argument struct
)
MIXED_CASES = [c for c in CASES if c.name == "mixed" and not c.offset]


def rows(sizes):
    """The chunk rows (tensor, first element), by the expression of train_step._adam_kernel_step."""
    return [(i, off) for i, n in enumerate(sizes) for off in range(0, n, CHUNK)]


# ---- the truth ------------------------------------------------------------------------------------------------------------------------
def adam64(p, g, m, v, step, h):
    """One Adam step with L2 weight decay from the definition, in float64; `step` is the count before the step."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    t = step + 1
    g = g + h.weight_decay * p
    m = h.beta1 * m + (1 - h.beta1) * g
    v = h.beta2 * v + (1 - h.beta2) * g * g
    bc1, bc2 = 1 - h.beta1 ** t, 1 - h.beta2 ** t
    denom = np.sqrt(v) / np.sqrt(bc2) + h.eps
    return p - h.lr / bc1 * m / denom, m, v


MUTANTS = ("step_not_plus_one", "no_weight_decay", "sq_before_decay", "decoupled_decay", "bc2_not_rooted", "eps_in_root",
           "eps_over_bc2")


def adam64_mutant(p, g, m, v, step, h, mutant):
    """adam64 with one mistake: the formulas a plausible wrong kernel would evaluate."""
    assert mutant in MUTANTS, mutant
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        t = step if mutant == "step_not_plus_one" else step + 1                      # bias corrections of the step before
        raw = g
        if mutant == "decoupled_decay":                                              # AdamW
            p = p * (1 - h.lr * h.weight_decay)
        elif mutant != "no_weight_decay":
            g = g + h.weight_decay * p
        m = h.beta1 * m + (1 - h.beta1) * g
        gv = raw if mutant == "sq_before_decay" else g                               # exp_avg_sq fed the undecayed gradient
        v = h.beta2 * v + (1 - h.beta2) * gv * gv
        bc1, bc2 = np.float64(1 - h.beta1 ** t), np.float64(1 - h.beta2 ** t)       # (numpy scalars: 0 divides to inf, no exception)
        if mutant == "bc2_not_rooted":
            denom = np.sqrt(v) / bc2 + h.eps
        elif mutant == "eps_in_root":
            denom = np.sqrt(v / bc2 + h.eps)
        elif mutant == "eps_over_bc2":
            denom = (np.sqrt(v) + h.eps) / np.sqrt(bc2)
        else:
            denom = np.sqrt(v) / np.sqrt(bc2) + h.eps
        return p - h.lr / bc1 * m / denom, m, v


def _walk(state, h, n_steps, one_step):
    out = {k: [] for k in NAMES}
    for p, g, m, v, s in zip(state["param"], state["grad"], state["exp_avg"], state["exp_avg_sq"], state["step"]):
        for k in range(n_steps):
            p, m, v = one_step(p, g, m, v, int(s) + k, h)
        for name, a in zip(NAMES, (p, m, v)):
            out[name].append(a)
    out["step"] = [int(s) + n_steps for s in state["step"]]
    return out


def truth(state, h, n_steps=1):
    """{param, exp_avg, exp_avg_sq: float64 arrays per tensor, step: counts} after n_steps steps with the same gradients."""
    return _walk(state, h, n_steps, adam64)


def mutated(state, h, mutant):
    return _walk(state, h, 1, functools.partial(adam64_mutant, mutant=mutant))


def mirror(state, h):
    """The expressions of adam_update_kernel with its rounding points: the bias corrections in double and handed on as fp32, every
    expression that mixes a double hyper-parameter with fp32 state in double and rounded once on assignment, the rest in fp32."""
    f32, f64 = np.float32, np.float64

    def one_step(p, g, m, v, s, h):
        step = f32(s) + f32(1)
        bc1 = f32(1.0 - h.beta1 ** float(step))
        bc2_sqrt = f32(math.sqrt(1.0 - h.beta2 ** float(step)))
        step_size = f32(h.lr / float(bc1))
        if h.weight_decay != 0.0:
            g = (g.astype(f64) + p.astype(f64) * h.weight_decay).astype(f32)
        m = (h.beta1 * m.astype(f64) + (1.0 - h.beta1) * g.astype(f64)).astype(f32)
        v = (h.beta2 * v.astype(f64) + (1.0 - h.beta2) * g.astype(f64) * g.astype(f64)).astype(f32)
        denom = ((np.sqrt(v) / bc2_sqrt).astype(f64) + h.eps).astype(f32)
        p = p - step_size * m / denom
        assert p.dtype == m.dtype == v.dtype == denom.dtype == f32
        return p, m, v

    return _walk(state, h, 1, one_step)


def torch_adam(state, h, dtype=torch.float32, n_steps=1):
    """torch.optim.Adam(foreach=False) on the host with the state injected: {param, exp_avg, exp_avg_sq, step} as torch tensors
    per tensor.  fp32: the yardstick; float64: an independent route to the truth."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).clone()  # noqa: E731
    params = [t(a).requires_grad_(True) for a in state["param"]]
    opt = torch.optim.Adam(params, lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, weight_decay=h.weight_decay, foreach=False)
    for p, g, m, v, s in zip(params, state["grad"], state["exp_avg"], state["exp_avg_sq"], state["step"]):
        p.grad = t(g)
        opt.state[p] = {"step": torch.tensor(float(s)), "exp_avg": t(m), "exp_avg_sq": t(v)}
    for _ in range(n_steps):
        opt.step()
    return {"param": [p.detach() for p in params], "exp_avg": [opt.state[p]["exp_avg"] for p in params],
            "exp_avg_sq": [opt.state[p]["exp_avg_sq"] for p in params], "step": [float(opt.state[p]["step"]) for p in params]}


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
def _tensor(c, i, n, h):
    rng = np.random.default_rng([c.seed, i, n, c.hyper, 4099])
    sign = lambda: rng.choice(np.float32([-1, 1]), n)  # noqa: E731
    p = rng.uniform(0.5, 1.5, n).astype(np.float32) * sign()
    g = rng.uniform(0.1, 1.0, n).astype(np.float32) * sign()
    if h.step0 == 0:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    gd = g.astype(np.float64) + h.weight_decay * p.astype(np.float64)
    m, v = np.empty(n, np.float32), np.empty(n, np.float32)
    todo_m = todo_v = np.arange(n)
    while todo_m.size or todo_v.size:       # (a draw is kept with probability > 0.9)
        m[todo_m] = rng.uniform(0.05, 0.5, todo_m.size).astype(np.float32) * np.sign(g[todo_m])
        v[todo_v] = rng.uniform(0.01, 0.5, todo_v.size).astype(np.float32)
        todo_m = todo_m[np.abs(gd[todo_m] - m[todo_m]) < MOMENT_GAP[0]]
        todo_v = todo_v[np.abs(gd[todo_v] ** 2 - v[todo_v]) < MOMENT_GAP[1]]
    return p, g, m, v


def decided_margin(state, tr):
    """{name: min over tensors of  min |truth - input| / (8 * 2**-24 * max|truth|)}: the least move of any element, in gate floors."""
    out = {}
    for name in NAMES:
        out[name] = min(float(np.abs(t - a.astype(np.float64)).min()) / (8 * U * float(np.abs(t).max()))
                        for a, t in zip(state[name], tr[name]))
    return out


@functools.lru_cache(maxsize=4)
def make(c):
    """dict: param, grad, exp_avg, exp_avg_sq (lists of fp32 numpy arrays, one per tensor), step (list of ints), hyper, truth
    (truth()), margin (decided_margin()).  Shared between tests: never written to."""
    h = HYPERS[c.hyper]
    d = {k: [] for k in NAMES + ("grad",)}
    for i, n in enumerate(c.sizes):
        for k, a in zip(("param", "grad", "exp_avg", "exp_avg_sq"), _tensor(c, i, n, h)):
            assert a.dtype == np.float32 and a.shape == (n,)
            d[k].append(a)
    d["step"] = [h.step0 + i % 3 for i in range(len(c.sizes))]
    d["hyper"] = h
    d["truth"] = truth(d, h)
    d["margin"] = decided_margin(d, d["truth"])
    for i in range(len(c.sizes)):
        p, g, m, v = (np.abs(d[k][i]) for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
        assert p.min() >= 0.5 and p.max() <= 1.5 and g.min() >= np.float32(0.1) and g.max() <= 1.0
        if h.step0 == 0:
            assert not m.any() and not v.any()
        else:
            assert m.min() >= np.float32(0.05) and m.max() <= 0.5 and np.array_equal(np.sign(d["exp_avg"][i]), np.sign(d["grad"][i]))
            assert d["exp_avg_sq"][i].min() >= np.float32(0.01) and v.max() <= 0.5
    assert min(d["margin"].values()) >= DECIDED, (case_id(c), d["margin"])
    return d
