"""include/ext/bunmpc_policy_train.h without a GPU: the header against its recorded table and a C compiler, the build job, the refusals
(they return before any launch), and the twin (bunmpc_amd/policy_train.py::host_step) -- held to the recording of the reference's own
network under the reference's loop one step at a time, to its own invariants, and the fit loop's plumbing on a stub."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bunmpc_amd import _lib, _lib_policy, _lib_policy_train, policy
from bunmpc_amd import build as hip_build
from bunmpc_amd import policy_train as pt
from tests import policy_cases
from tests import policy_train_cases as cases
from tests.policy_train_cases import same_bits
from tests.test_abi_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_abi  # noqa: E402

EXT = os.path.dirname(_lib_policy_train.HEADER)
STEPS = [(i, k) for i in range(3) for k in cases.steps_of(i)]


# ---- the header and the job ------------------------------------------------------------------------------------------------------------

def test_header_equals_its_recorded_table():
    with open(os.path.join(ROOT, "tests", "golden", "abi_policy_train.json")) as f:
        assert record_abi.dump(_lib_policy_train.ABI) == f.read()
    assert sorted(_lib_policy_train.ABI.functions) == ["bmpc_policy_pack_device", "bmpc_policy_params_struct_size", "bmpc_policy_step_struct_size", "bmpc_policy_train_step_device",
                                                       "bmpc_policy_train_struct_size", "bmpc_policy_train_tile", "bmpc_policy_train_work_bytes"]
    assert _lib_policy_train.PAD == _lib_policy.PAD == 16 and _lib_policy_train.MAX_ROWS == 1024


def test_job_sits_directly_after_the_policy_with_its_flags():
    assert _lib_policy_train.HEADER in hip_build.dependencies() and "bunmpc_policy_train.h" not in _lib.HEADER_NAMES
    assert not set(_lib_policy_train.ABI.functions) & (set(_lib._SIGS) | set(_lib_policy.ABI.functions))
    assert not set(_lib_policy_train.ABI.structs) & (set(_lib._ABI.structs) | set(_lib_policy.ABI.structs))
    jobs = hip_build.compile_jobs()
    job = hip_build.job("policy_train")
    assert jobs.index(job) == jobs.index(hip_build.job("policy")) + 1 and jobs.index(job) < jobs.index(hip_build.job("acyclic_plan")) and job in jobs[12:-2]
    assert job[1] == "policy_train.hip" and job[2] == hip_build.job("policy")[2] == hip_build._POLICY_FLAGS
    assert "-fno-fast-math" in job[2] and "-fno-gpu-flush-denormals-to-zero" in job[2] and "-ffp-contract=off" in job[2]
    lib = _lib_policy_train.lib()      # the symbols are in the library, with the header's struct sizes
    for cname, cls in _lib_policy_train.ABI.structs.items():
        assert getattr(lib, cname[:-2] + "_struct_size")() == C.sizeof(cls)
    assert lib.bmpc_policy_train_tile() % 16 == 0 and 16 <= lib.bmpc_policy_train_tile() <= 1024


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip("no C compiler on this machine")
    want, lines = [], []
    for cname, cls in _lib_policy_train.ABI.structs.items():
        want.append("%s %d" % (cname, C.sizeof(cls)))
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            want.append("%s.%s %d %d" % (cname, field, getattr(cls, field).offset, getattr(cls, field).size))
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, field, cname, field, cname, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bunmpc_policy_train.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", EXT, "-o", str(tmp_path / "layout"), str(src)])
    assert subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")[:-1] == want
    for lang in ("c", "c++"):      # alone, as C and as C++; and it includes nothing
        subprocess.check_call([cc, "-x", lang, "-fsyntax-only", "-Wall", "-Werror", _lib_policy_train.HEADER])
    assert "#include" not in open(_lib_policy_train.HEADER).read()
    both = tmp_path / "both.c"      # and beside the first header and the forward pass's
    both.write_text('#include "bunmpc.h"\n#include "ext/bunmpc_dataset.h"\n#include "ext/bunmpc_policy.h"\n#include "ext/bunmpc_policy_train.h"\nint main(void) { return 0; }\n')
    subprocess.check_call([cc, "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.dirname(hip_build.INCLUDE), str(both)])


# ---- refusals: before anything is written or launched, so they need no GPU ----------------------------------------------------------------

def _set(d, kw):
    for k, v in kw.items():
        if "." in k or "[" in k:      # "m.W[1]", "running_var[0]"
            head, _, index = k.partition("[")
            obj = d
            for part in head.split(".")[:-1]:
                obj = getattr(obj, part)
            getattr(obj, head.split(".")[-1])[int(index[:-1])] = v
        else:
            setattr(d, k, v)
    return d


def _net(**kw):
    """a descriptor that passes every check (its arrays are never touched: every call below is refused), with fields replaced"""
    d = _lib_policy_train.PolicyTrain()
    d.n_in, d.n_hidden, d.n_layers, d.n_out, d.batch_norm, d.eps = 55, 64, 2, 12, 1, 1e-5
    for q in (d.p, d.m, d.v):
        for l in range(9):
            q.W[l] = q.b[l] = 4096
        for l in range(8):
            q.gamma[l] = q.beta[l] = 4096
    for l in range(8):
        d.running_mean[l] = d.running_var[l] = 4096
    d.work, d.work_bytes = 4096, 1 << 30
    return _set(d, kw)


_GRADS = _lib_policy_train.PolicyParams()


def _step(**kw):
    s = _lib_policy_train.PolicyStep()
    s.n, s.x, s.y, s.loss, s.x_stride, s.y_stride, s.lr, s.bc1, s.bc2 = 16, 4096, 4096, 4096, 55, 12, 0.002, 0.1, 0.001
    return _set(s, kw)


def _call(net, step):
    return _lib_policy_train.lib().bmpc_policy_train_step_device(C.byref(net) if net is not None else None, C.byref(step) if step is not None else None, None)


@pytest.mark.parametrize("kw,word", [(dict(n_layers=0), "n_layers"), (dict(n_layers=9), "n_layers"), (dict(n_in=0), "n_in"), (dict(n_in=513), "n_in"),
                                     (dict(n_hidden=0), "n_hidden"), (dict(n_hidden=513), "n_hidden"), (dict(n_out=0), "n_out"), (dict(n_out=65), "n_out"),
                                     ({"p.W[0]": None}, "p.W[0]"), ({"p.b[2]": None}, "p.b[2]"), ({"p.gamma[1]": None}, "p.gamma[1]"), ({"p.beta[0]": None}, "p.beta[0]"),
                                     ({"running_mean[1]": None}, "running_mean[1]"), ({"running_var[0]": None}, "running_var[0]"),
                                     (dict(eps=-1e-5), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=float("inf")), "eps")])
def test_step_and_packer_refuse_a_bad_network_and_name_the_field(kw, word):
    assert _call(_net(**kw), _step()) == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()
    assert _lib_policy_train.lib().bmpc_policy_pack_device(C.byref(_net(**kw)), 4096, 64, None) == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("net_kw,kw,word", [({}, dict(n=0), "n must be"), ({}, dict(n=1025), "n must be"), ({}, dict(n=-1), "n must be"), ({}, dict(n=1), "batch_norm"),
                                            ({}, dict(x=None), "array: x"), ({}, dict(y=None), "array: y"), ({}, dict(loss=None), "loss"),
                                            ({}, dict(x_stride=54), "x_stride"), ({}, dict(y_stride=11), "y_stride"),
                                            ({}, dict(lr=float("nan")), "lr must be"), ({}, dict(lr=float("inf")), "lr must be"), ({}, dict(bc1=0.0), "bc1"), ({}, dict(bc2=float("nan")), "bc2"), ({}, dict(bc2=-1.0), "bc2"),
                                            ({"m.W[1]": None}, {}, "m.W[1]"), ({"v.b[0]": None}, {}, "v.b[0]"), ({"v.gamma[0]": None}, {}, "v.gamma[0]"),
                                            (dict(work=None), {}, "work"), (dict(work=4104), {}, "work must be 16-byte"), (dict(work_bytes=1024), {}, "work_bytes"),
                                            ({}, dict(grads=C.addressof(_GRADS)), "grads.W[0]")])
def test_step_refusals_name_the_field(net_kw, kw, word):
    assert _call(_net(**net_kw), _step(**kw)) == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


def test_further_refusals_and_the_sizes():
    lib = _lib_policy_train.lib()
    assert _call(None, _step()) == _lib.BAD_ARG and "null network descriptor" in _lib.last_error()
    assert _call(_net(), None) == _lib.BAD_ARG and "step descriptor" in _lib.last_error()
    # without batch_norm one row is a batch, and gamma, beta and the running statistics are not looked at: only the scratch is missing here
    plain = _net(batch_norm=0, work=None, **{"p.gamma[0]": None, "running_mean[0]": None})
    assert _call(plain, _step(n=1)) == _lib.BAD_ARG and "work" in _lib.last_error()
    # the packer: the image's size, address and alignment; Adam's moments are not looked at
    want = _lib_policy.lib().bmpc_policy_packed_bytes(55, 64, 2, 12, 1)
    assert lib.bmpc_policy_pack_device(None, 4096, want, None) == _lib.BAD_ARG and "null network descriptor" in _lib.last_error()
    assert lib.bmpc_policy_pack_device(C.byref(_net()), 4096, want - 4, None) == _lib.BAD_ARG and "packed_bytes" in _lib.last_error() and str(want) in _lib.last_error()
    assert lib.bmpc_policy_pack_device(C.byref(_net()), None, want, None) == _lib.BAD_ARG and "null packed image" in _lib.last_error()
    assert lib.bmpc_policy_pack_device(C.byref(_net()), 4104, want, None) == _lib.BAD_ARG and "16-byte aligned" in _lib.last_error()
    assert lib.bmpc_policy_pack_device(C.byref(_net(**{"m.W[0]": None})), None, want, None) == _lib.BAD_ARG and "null packed image" in _lib.last_error()
    # the scratch: per row a_0 .. a_L, the prediction and two dz buffers; BatchNorm adds xhat per hidden layer and invstd
    r4 = lambda v: (v + 3) // 4 * 4      # noqa: E731
    for n in (1, 40, 1024):
        plain = 4 * (r4(55 * n) + 2 * r4(64 * n) + r4(12 * n) + 2 * r4(64 * n))
        assert lib.bmpc_policy_train_work_bytes(55, 64, 2, 12, 0, n) == plain
        assert lib.bmpc_policy_train_work_bytes(55, 64, 2, 12, 1, n) == plain + 4 * 2 * (r4(64 * n) + 64)
    for args in ((0, 64, 2, 12, 0, 8), (55, 513, 2, 12, 0, 8), (55, 64, 9, 12, 0, 8), (55, 64, 2, 65, 0, 8), (55, 64, 2, 12, 0, 0), (55, 64, 2, 12, 0, 1025)):
        assert lib.bmpc_policy_train_work_bytes(*args) == -1


# ---- the twin against the recording of the reference's loop, one step at a time ------------------------------------------------------------

def _error(got, want64):
    """E: max |got - want| over every entry of every array jointly, over max |want| -- one global scale"""
    got, want64 = (np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in v]) for v in (got, want64))
    return np.abs(got - want64).max() / np.abs(want64).max()


@pytest.mark.parametrize("i,k", STEPS)
def test_gradients_are_as_close_to_float64_as_the_reference_s(i, k):
    """E(g) = max over every parameter of |g - g64| / max |g64|, one global scale (with BatchNorm the bias of the Linear ahead of it has a
    gradient that is zero in exact arithmetic and rounding noise in fp32); g64 is the reference's own step in float64 from the same fp32
    state.  Criterion: E(twin) <= 8 E(torch fp32), the factor for serial chains over 40 rows against torch's blocked sums.  Measured on
    the ten recorded steps: E(twin) 1.2e-7 .. 4.9e-7, E(torch fp32) 1.5e-7 .. 5.0e-7, ratio 0.73 .. 1.84."""
    c = cases.recorded(i, k)
    g64 = c["g"].astype(np.float64) + c["d"].astype(np.float64)
    e_twin, e_ref = _error([cases.vector(cases.twin_step(i, k)[2])], [g64]), _error([c["g"]], [g64])
    print("net %d step %d: E(twin) %.3e, E(torch fp32) %.3e, ratio %.2f" % (i, k, e_twin, e_ref, e_twin / e_ref))
    assert e_ref > 0 and e_twin <= 8 * e_ref


@pytest.mark.parametrize("i,k", STEPS)
def test_predictions_and_statistics_are_as_close_to_float64_as_the_reference_s(i, k):
    """the same criterion on the predictions, on the batch's mean and biased variance, and on the running statistics after the step, each
    over all its entries jointly.  Measured ratios: predictions 0.82 .. 1.21, batch statistics 1.29 .. 3.11 (torch's figure here is its own mean and var of the values
    entering BatchNorm1d), running statistics 0.76 .. 1.00."""
    c = cases.recorded(i, k)
    state, _, _, fwd = cases.twin_step(i, k)
    p64 = c["pred"].astype(np.float64) + c["dpred"].astype(np.float64)
    checks = [("predictions", [fwd["p"]], [c["pred"]], [p64])]
    if c["dims"][4]:
        checks.append(("batch statistics", [np.stack(fwd["mean"]), np.stack(fwd["var"])], [c["bmean"], c["bvar"]], [c["dbmean"], c["dbvar"]]))
        checks.append(("running statistics", [np.stack(state.running_mean), np.stack(state.running_var)], [c["rm"], c["rv"]], [c["drm"], c["drv"]]))
    for name, twin, ref, want in checks:
        e_twin, e_ref = _error(twin, want), _error(ref, want)
        print("net %d step %d, %s: E(twin) %.3e, E(torch fp32) %.3e, ratio %.2f" % (i, k, name, e_twin, e_ref, e_twin / e_ref))
        assert e_ref > 0 and e_twin <= 8 * e_ref, name


@pytest.mark.parametrize("i,k", STEPS)
def test_loss_is_the_float64_mean_of_the_twin_s_predictions(i, k):
    c = cases.recorded(i, k)
    _, loss, _, fwd = cases.twin_step(i, k)
    want = np.mean(np.abs(fwd["p"].astype(np.float64) - c["y"]))
    assert abs(loss - want) <= fwd["p"].size * 2.0 ** -53 * want
    assert abs(loss - float(c["dloss"])) < 1e-6 and abs(loss - float(c["loss"])) < 1e-6      # and it is the reference's loss


def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float32))).astype(np.float64)


@pytest.mark.parametrize("i,k", STEPS)
def test_adam_rule_alone_gives_the_reference_s_state(i, k):
    """host_adam on the reference's own fp32 gradients and before-state, t = 1, 2, 3 and 1000: exp_avg and exp_avg_sq within 4 fp32 ulps
    (measured: 0), the parameters within ulp32(p) + 8 * 2^-24 |p_after - p_before| -- the rule's handful of fp32 roundings, each relative
    to the update, and the final rounding of p."""
    c = cases.recorded(i, k)
    before = c["before"]
    p, m, v = (cases.vector(q).astype(np.float64) for q in pt.host_adam(before.p, cases.params(c["dims"], c["g"]), before.m, before.v, c["lr"], c["t"]))
    assert np.all(np.abs(m - c["m"]) <= 4 * _ulp32(c["m"])) and np.all(np.abs(v - c["v"]) <= 4 * _ulp32(c["v"]))
    moved = np.abs(c["p"].astype(np.float64) - cases.vector(before.p))
    assert np.all(np.abs(p - c["p"]) <= _ulp32(c["p"]) + 8 * 2.0 ** -24 * moved)
    assert moved.max() > 0.5 * c["lr"] and (k != 1000 or abs(pt.bias_corrections(c["t"])[1] - 0.632) < 1e-3)


def test_recorded_steps_are_consecutive_and_clear_of_every_kink():
    """the state after step k is the state before step k + 1, and (the generator's assertion, seen from here) no value entering a ReLU
    and no p - y of the twin is closer to 0 than 0.9e-4"""
    for i, k in STEPS:
        c = cases.recorded(i, k)
        fwd = cases.twin_step(i, k)[3]
        assert np.abs(fwd["p"] - c["y"]).min() > 0.9e-4
        assert all(np.abs(a[a != 0]).min() > 0.9e-4 for a in fwd["a"][1:])
    assert same_bits(cases.vector(cases.recorded(2, 2)["before"].m), cases.recording()["n2_s1_m"])
    assert same_bits(cases.vector(cases.recorded(0, 1000)["before"].p), cases.recording()["n0_s2_p"])
    assert os.path.getsize(cases.GOLDEN) < 1 << 20      # a committed file stays under 1 MiB


# ---- the twin's own invariants ----------------------------------------------------------------------------------------------------------------

def _embedded(net, extra_in, extra_hidden):
    """`net` with extra input columns and extra hidden units whose weights and biases are +0: the padding a wider layout would hold"""
    H, L = net.n_hidden + extra_hidden, net.n_layers
    W, b = [], []
    for l in range(L + 1):
        N, K = (net.n_out if l == L else H), (net.n_in + extra_in if l == 0 else H)
        w, v = np.zeros((N, K), np.float32), np.zeros(N, np.float32)
        w[:net.W[l].shape[0], :net.W[l].shape[1]], v[:net.b[l].shape[0]] = net.W[l], net.b[l]
        W.append(w)
        b.append(v)
    return policy.PolicyNet.from_arrays(W, b)


def test_padding_gets_zero_gradient_and_stays_zero_through_adam():
    net, x, y = cases.drawn(31, 23, 24, 2, 12, False, 19)
    wide = _embedded(net, 3, 5)
    xw = np.hstack((x, np.zeros((19, 3))))
    state, loss, g = pt.host_step(pt.TrainState.from_net(net), x, y, 0.002, 1)
    state_w, loss_w, g_w = pt.host_step(pt.TrainState.from_net(wide), xw, y, 0.002, 1)
    assert same_bits(np.float64(loss), np.float64(loss_w))
    for l in range(3):
        N, K = net.W[l].shape
        for got, inner in ((g_w.W[l], g.W[l]), (state_w.p.W[l], state.p.W[l]), (state_w.m.W[l], state.m.W[l]), (state_w.v.W[l], state.v.W[l])):
            assert same_bits(got[:N, :K], inner)
            outside = np.concatenate((got[N:].reshape(-1), got[:, K:].reshape(-1)))
            assert not outside.any() and not np.signbit(outside).any()
        for got, inner in ((g_w.b[l], g.b[l]), (state_w.p.b[l], state.p.b[l])):
            assert same_bits(got[:N], inner) and not got[N:].any() and not np.signbit(got[N:]).any()
    # padded rows: a chain over 19 rows ends with the +0 terms of rows 19 .. 31, which change no bit of a chain that started from +0
    assert same_bits(pt.chain(np.float32(x)), pt.chain(np.vstack((np.float32(x), np.zeros((13, 23), np.float32)))))


@pytest.mark.parametrize("bn", [False, True])
def test_a_nan_in_one_row_reaches_the_loss_and_every_gradient(bn):
    net, x, y = cases.drawn(37, 23, 24, 2, 12, bn, 19)
    x[7, 3] = np.nan
    state, loss, g = pt.host_step(pt.TrainState.from_net(net), x, y, 0.002, 1)
    assert np.isnan(loss) and all(np.all(np.isnan(a)) for _, a in g.arrays()) and all(np.all(np.isnan(a)) for _, a in state.p.arrays())


def test_smallest_batches():
    net, x, y = cases.drawn(41, 23, 24, 2, 12, True, 2)
    state, loss, g = pt.host_step(pt.TrainState.from_net(net), x, y, 0.002, 1)
    assert np.isfinite(loss) and all(np.all(np.isfinite(a)) for _, a in cases.state_fields(state))
    with pytest.raises(ValueError):
        pt.host_step(pt.TrainState.from_net(net), x[:1], y[:1], 0.002, 1)
    plain, x, y = cases.drawn(43, 23, 24, 2, 12, False, 1)
    state, loss, g = pt.host_step(pt.TrainState.from_net(plain), x, y, 0.002, 1)
    # one row: db of the output layer is the row's signs over n_out, and the loss its mean
    assert same_bits(g.b[-1], np.sign(policy.host_forward(plain, x) - np.float32(y))[0] * pt.div32(1, np.float32(12)))
    assert loss == np.mean(np.abs(policy.host_forward(plain, x).astype(np.float64) - np.float32(y)))


@pytest.mark.parametrize("bn", [False, True])
def test_state_dict_loads_into_torch_and_the_packer_takes_the_trained_net(bn):
    import torch
    net, x, y = cases.drawn(47, 23, 24, 2, 12, bn, 19)
    trainer = pt.HostTrainer(net, lr=0.002)
    trainer.step(x, y)
    trainer.step(x, y)
    trained = trainer.net()
    layers = []
    for l in range(2):
        layers += [torch.nn.Linear(23 if l == 0 else 24, 24)] + ([torch.nn.BatchNorm1d(24)] if bn else []) + [torch.nn.ReLU()]
    module = torch.nn.Module()
    module.net = torch.nn.Sequential(*layers, torch.nn.Linear(24, 12))
    sd = {key: torch.from_numpy(np.array(v)) for key, v in pt.state_dict_arrays(trained, trainer.t).items()}
    assert list(sd) == list(module.state_dict())
    module.load_state_dict(sd)      # strict
    if bn:
        assert int(module.net[1].num_batches_tracked) == 2
    with torch.no_grad():
        got = module.eval().net(torch.from_numpy(np.float32(x))).numpy()
    assert np.abs(got - policy.host_forward(trained, x)).max() < 1e-5
    again = policy.PolicyNet.from_state_dict({key: v for key, v in sd.items() if not key.endswith("num_batches_tracked")}, eps=trained.eps)
    assert same_bits(policy.pack(again), policy.pack(trained))
    for l, (W, b, s, t) in enumerate(policy.unpack(trained.dims, policy.pack(trained))):
        N, K = trained.W[l].shape
        assert same_bits(W[:N, :K], trainer.state.p.W[l]) and same_bits(b[:N], trainer.state.p.b[l])
        if bn and l < 2:
            assert same_bits(s[:N], trained.scale_shift(l)[0]) and same_bits(t[:N], trained.scale_shift(l)[1])
    assert not same_bits(policy.pack(trained), policy.pack(net))


def test_a_planted_fault_breaks_the_bitwise_comparison():
    """what the GPU tests rely on: a step that takes its row sums descending, or Adam's count one too high, differs in some bit"""
    c = cases.recorded(2, 0)
    state, loss, g, _ = cases.twin_step(2, 0)
    assert cases.first_difference(state, pt.host_step(c["before"], c["x"], c["y"], c["lr"], c["t"])[0]) is None
    flipped = pt.host_step(c["before"], c["x"][::-1], c["y"][::-1], c["lr"], c["t"])
    assert cases.first_difference(flipped[0], state, flipped[2], g) is not None
    assert cases.first_difference(pt.host_step(c["before"], c["x"], c["y"], c["lr"], c["t"] + 1)[0], state) == "p.W0"


# ---- fit's plumbing on a stub -------------------------------------------------------------------------------------------------------------------

class _StubRows:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def batch(self, index):
        return np.asarray(index), None


class _StubTrainer(pt._Loop):
    n_out = 12

    def __init__(self):
        self.steps, self.valid = [], []

    def step(self, x, y):
        self.steps.append(x)
        return float(len(self.steps))

    def l1_rows(self, x, y):
        self.valid.append(x)
        return np.full(len(x), 6.0)

    def _read(self, losses, errs):
        return np.concatenate([np.asarray(losses, np.float64)] + errs)


def test_fit_plumbing():
    trainer = _StubTrainer()
    history = trainer.fit(_StubRows(1000), n_epoch=3, batch_size=64, n_train_frac=0.9, seed=5)
    epochs, valid = pt.fit_indices(1000, 3, 64, 0.9, 5)
    # the split: 900 and 100 rows, disjoint, together every row
    train_rows = np.unique(np.concatenate(epochs[0]))
    assert len(valid) == 100 and len(np.unique(valid)) == 100 and not set(valid) & set(train_rows) and set(valid) | set(np.concatenate(trainer.steps)) <= set(range(1000))
    # drop_last: 14 batches of 64 per epoch, no short one; every epoch draws from the same 900 training rows
    assert [len(e) for e in epochs] == [14, 14, 14] and all(len(b) == 64 for e in epochs for b in e) and len(trainer.steps) == 42
    assert all(len(np.unique(np.concatenate(e))) == 14 * 64 and not set(np.concatenate(e)) & set(valid) for e in epochs)
    # a new permutation each epoch
    assert not np.array_equal(np.concatenate(epochs[0]), np.concatenate(epochs[1])) and not np.array_equal(np.concatenate(epochs[1]), np.concatenate(epochs[2]))
    # the loop ran what fit_indices lists, validation after every epoch over every validation row, in chunks of the batch size
    assert all(np.array_equal(a, b) for a, b in zip(trainer.steps, [b for e in epochs for b in e]))
    assert [len(v) for v in trainer.valid] == [64, 36] * 3 and np.array_equal(np.concatenate(trainer.valid[:2]), valid)
    assert history == [(np.mean(np.arange(14 * e + 1, 14 * e + 15)), 0.5) for e in range(3)]
    # the same seed gives the same sequence, another seed another
    again, valid_again = pt.fit_indices(1000, 3, 64, 0.9, 5)
    assert np.array_equal(valid, valid_again) and all(np.array_equal(a, b) for ea, eb in zip(epochs, again) for a, b in zip(ea, eb))
    assert not np.array_equal(valid, pt.fit_indices(1000, 3, 64, 0.9, 6)[1])
    # fewer training rows than a batch: no step, and no validation row: NaN
    empty = _StubTrainer()
    assert np.isnan(empty.fit(_StubRows(50), n_epoch=1, batch_size=64, n_train_frac=1.0, seed=0)[0]).all() and not empty.steps
