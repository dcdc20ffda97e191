"""include/ext/bunmpc_policy.h without a GPU: the header against its recorded table and a C compiler, the build job, the refusals (they
return before any launch), the packer against an unpack helper, and the twin (bunmpc_amd/policy.py::host_forward) -- its array fma held
to exact rationals, its results to the recording of the reference's own network, and shown to fail, with one fault planted, the
bitwise comparison the GPU tests apply."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from bunmpc_amd import _lib, _lib_policy, policy
from bunmpc_amd import build as hip_build
from tests import policy_cases as cases
from tests.policy_cases import same_bits
from tests.test_abi_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_abi  # noqa: E402

EXT = os.path.dirname(_lib_policy.HEADER)


# ---- the header and the job ------------------------------------------------------------------------------------------------------------

def test_header_equals_its_recorded_table():
    with open(os.path.join(ROOT, "tests", "golden", "abi_policy.json")) as f:
        assert record_abi.dump(_lib_policy.ABI) == f.read()
    assert sorted(_lib_policy.ABI.functions) == ["bmpc_policy_forward_device", "bmpc_policy_net_struct_size", "bmpc_policy_pack_host", "bmpc_policy_packed_bytes",
                                                 "bmpc_policy_rows_struct_size", "bmpc_policy_tile", "bmpc_policy_weights_struct_size"]
    assert (_lib_policy.STATE_WIDTH, _lib_policy.Q_WIDTH, _lib_policy.V_WIDTH, _lib_policy.TAU_WIDTH) == (43, 19, 18, 12)


def test_job_sits_among_the_side_units_with_its_flags():
    assert _lib_policy.HEADER in hip_build.dependencies() and "bunmpc_policy.h" not in _lib.HEADER_NAMES
    assert not set(_lib_policy.ABI.functions) & set(_lib._SIGS) and not set(_lib_policy.ABI.structs) & set(_lib._ABI.structs)
    jobs = hip_build.compile_jobs()
    job = hip_build.job("policy")
    assert job in jobs[12:-2] and job[1] == "policy.hip" and jobs.index(job) < jobs.index(hip_build.job("acyclic_plan"))
    assert "-fno-fast-math" in job[2] and "-fno-gpu-flush-denormals-to-zero" in job[2] and "-ffp-contract=off" in job[2]
    assert not any(f in job[2] for f in ("-ffast-math", "-fgpu-flush-denormals-to-zero", "-Ofast", "-funsafe-math-optimizations"))
    lib = _lib_policy.lib()      # the symbols are in the library, with the header's struct sizes
    assert lib.bmpc_policy_net_struct_size() == C.sizeof(_lib_policy.PolicyNetDesc) and lib.bmpc_policy_rows_struct_size() == C.sizeof(_lib_policy.PolicyRows)
    assert lib.bmpc_policy_weights_struct_size() == C.sizeof(_lib_policy.PolicyWeights)
    assert lib.bmpc_policy_tile() % 16 == 0 and lib.bmpc_policy_tile() >= 16


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip("no C compiler on this machine")
    want, lines = [], []
    for cname, cls in _lib_policy.ABI.structs.items():
        want.append("%s %d" % (cname, C.sizeof(cls)))
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            want.append("%s.%s %d %d" % (cname, field, getattr(cls, field).offset, getattr(cls, field).size))
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, field, cname, field, cname, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bunmpc_policy.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", EXT, "-o", str(tmp_path / "layout"), str(src)])
    assert subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")[:-1] == want
    for lang in ("c", "c++"):      # alone, as C and as C++; and it includes nothing
        subprocess.check_call([cc, "-x", lang, "-fsyntax-only", "-Wall", "-Werror", _lib_policy.HEADER])
    assert "#include" not in open(_lib_policy.HEADER).read()
    both = tmp_path / "both.c"      # and beside the first header and the others under ext/
    both.write_text('#include "bunmpc.h"\n#include "ext/bunmpc_acyclic.h"\n#include "ext/bunmpc_dataset.h"\n#include "ext/bunmpc_contact_log.h"\n'
                    '#include "ext/bunmpc_policy.h"\nint main(void) { return 0; }\n')
    subprocess.check_call([cc, "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.dirname(hip_build.INCLUDE), str(both)])


# ---- refusals: before anything is written or launched, so they need no GPU ----------------------------------------------------------------

def _set(d, kw):
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _net(**kw):
    """a descriptor that passes every check (its image is never touched: every call below is refused), with fields replaced"""
    d = _lib_policy.PolicyNetDesc()
    d.n_in, d.n_hidden, d.n_layers, d.n_out, d.batch_norm = 55, 64, 2, 12, 0
    d.packed = 4096
    _set(d, {k: v for k, v in kw.items() if k != "packed_bytes"})
    d.packed_bytes = max(_lib_policy.lib().bmpc_policy_packed_bytes(d.n_in, d.n_hidden, d.n_layers, d.n_out, d.batch_norm), 0)
    return _set(d, kw)


def _rows(**kw):
    """form 2 with every output; x=4096 switches to form 1"""
    r = _lib_policy.PolicyRows()
    r.n = 16
    r.state = r.goal = r.mean = r.std = r.action = r.tau = r.q = r.v = r.err = r.label = 4096
    r.state_stride, r.goal_stride, r.q_stride, r.v_stride, r.label_stride, r.x_stride = 43, 12, 19, 18, 12, 55
    r.action_type = _lib_policy.ACTION_TYPE["pd_target"]
    if "x" in kw:
        r.state = r.goal = r.mean = r.std = None
    return _set(r, kw)


def _forward(net, rows):
    return _lib_policy.lib().bmpc_policy_forward_device(C.byref(net) if net is not None else None, C.byref(rows) if rows is not None else None, None)


@pytest.mark.parametrize("kw,word", [(dict(n_layers=0), "n_layers"), (dict(n_layers=9), "n_layers"), (dict(n_in=0), "n_in"), (dict(n_in=513), "n_in"),
                                     (dict(n_hidden=0), "n_hidden"), (dict(n_hidden=513), "n_hidden"), (dict(n_out=0), "n_out"), (dict(n_out=65), "n_out"),
                                     (dict(packed=None), "packed"), (dict(packed=4104), "packed"), (dict(packed_bytes=64), "packed_bytes")])
def test_forward_and_packer_refuse_a_bad_network_and_name_the_field(kw, word):
    assert _forward(_net(**kw), _rows()) == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()
    w = _lib_policy.PolicyWeights()
    assert _lib_policy.lib().bmpc_policy_pack_host(C.byref(_net(**kw)), C.byref(w)) == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("kw,word", [(dict(n=-1), "n must be"), (dict(n=1 << 31), "n must be"), (dict(x=4096, state=4096), "both input forms"),
                                     (dict(state=None, goal=None), "neither x nor"), (dict(state=None), "array: state"), (dict(goal=None), "array: goal"),
                                     (dict(x=4096, x_stride=54), "x_stride"), (dict(state_stride=42), "state_stride"), (dict(goal_stride=11), "goal_stride"),
                                     (dict(q_stride=18), "q_stride"), (dict(v_stride=17), "v_stride"), (dict(label_stride=11), "label_stride"),
                                     (dict(mean=None), "null mean"), (dict(std=None), "null std"), (dict(x=4096, mean=4096, std=4096), "mean / std"),
                                     (dict(action_type=3), "action_type"), (dict(action_type=-1), "action_type"),
                                     (dict(action_type=2), "n_out"), (dict(q=None), "array: q"), (dict(v=None), "array: v"), (dict(label=None), "array: label")])
def test_forward_refusals_name_the_field(kw, word):
    assert _forward(_net(), _rows(**kw)) == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


def test_further_refusals_and_the_sizes():
    lib = _lib_policy.lib()
    assert _forward(None, _rows()) == _lib.BAD_ARG and "null network descriptor" in _lib.last_error()
    assert _forward(_net(), None) == _lib.BAD_ARG and "rows descriptor" in _lib.last_error()
    # tau's type against n_out, both ways; the state, goal form needs a goal
    for n_out, action_type in ((36, "pd_target"), (36, "torque"), (12, "structured"), (13, "torque")):
        assert _forward(_net(n_out=n_out), _rows(action_type=_lib_policy.ACTION_TYPE[action_type])) == _lib.BAD_ARG and "n_out" in _lib.last_error()
    assert _forward(_net(n_in=43), _rows()) == _lib.BAD_ARG and "w_goal" in _lib.last_error()
    assert lib.bmpc_policy_pack_host(C.byref(_net()), None) == _lib.BAD_ARG and "weights descriptor" in _lib.last_error()
    w = _lib_policy.PolicyWeights()
    assert lib.bmpc_policy_pack_host(C.byref(_net()), C.byref(w)) == _lib.BAD_ARG and "W[0]" in _lib.last_error()
    for l in range(3):
        w.W[l] = w.b[l] = 4096
    assert lib.bmpc_policy_pack_host(C.byref(_net(batch_norm=1)), C.byref(w)) == _lib.BAD_ARG and "gamma[0]" in _lib.last_error()
    for args in ((0, 64, 2, 12, 0), (513, 64, 2, 12, 0), (55, 0, 2, 12, 0), (55, 513, 2, 12, 0), (55, 64, 0, 12, 0), (55, 64, 9, 12, 0), (55, 64, 2, 0, 0), (55, 64, 2, 65, 0)):
        assert lib.bmpc_policy_packed_bytes(*args) == -1
    # K and N padded to 16: (64 x 64 + 64) + (64 x 64 + 64) + (16 x 64 + 16) floats; BatchNorm adds s and t per hidden layer
    assert lib.bmpc_policy_packed_bytes(55, 64, 2, 12, 0) == 4 * (2 * (64 * 64 + 64) + 16 * 64 + 16)
    assert lib.bmpc_policy_packed_bytes(55, 64, 2, 12, 1) == 4 * (2 * (64 * 64 + 3 * 64) + 16 * 64 + 16)
    assert lib.bmpc_policy_packed_bytes(512, 512, 8, 64, 1) > 0
    # the constructors refuse what the library would
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError):
        policy.pack(cases.random_net(rng, 55, 600, 1, 12))
    with pytest.raises(ValueError):
        policy.PolicyNet.from_arrays([np.zeros((8, 5)), np.zeros((3, 7))], [np.zeros(8), np.zeros(3)])
    with pytest.raises(ValueError):
        policy.host_input(cases.recorded(0)[0], x=np.zeros((2, 48)), mean=np.zeros(48), std=np.ones(48))


# ---- the array fma against exact rationals --------------------------------------------------------------------------------------------------

def _round_f32(x):
    """the float32 nearest to the Fraction x, ties to even, subnormals included (|x| < 2^128)"""
    if x == 0:
        return 0.0
    sign, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)
    n = x / q
    r = n.numerator // n.denominator
    rest = n - r
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and r % 2):
        r += 1
    return sign * float(r * q)


def test_array_fma_against_exact_rationals():
    """12000 triples: half with c within a few ulps of -a b, so the sum cancels to the bits the product's rounding would lose; magnitudes
    from the subnormal range to 1e15"""
    rng = np.random.default_rng(42)
    n = 12000
    a = (rng.normal(size=n) * 10.0 ** rng.uniform(-22, 7, size=n)).astype(np.float32)
    b = (rng.normal(size=n) * 10.0 ** rng.uniform(-22, 7, size=n)).astype(np.float32)
    c = (rng.normal(size=n) * 10.0 ** rng.uniform(-44, 15, size=n)).astype(np.float32)
    near = -(a[:n // 2].astype(np.float64) * b[:n // 2].astype(np.float64)).astype(np.float32)
    steps = np.where(np.abs(near) > 1e-37, rng.integers(-3, 4, size=n // 2), 0).astype(np.int32)      # (not across zero: those bits are NaNs)
    c[:n // 2] = (near.view(np.int32) + steps).view(np.float32)
    # 2^23 + 1 + (1/2 - 2^-41): float64 rounds the sum onto the float32 tie, and the tie then goes up to the even neighbour; the fma stays
    a[-1], b[-1], c[-1] = np.float32(1 + 2.0 ** -20), np.float32(0.5 - 2.0 ** -21), np.float32(2.0 ** 23 + 1)
    assert np.all(np.isfinite(c)) and np.all(a != 0) and np.all(b != 0)
    got = policy.fma32(a, b, c)
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want), np.argwhere(got != want)[:4]
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)      # rounded twice
    assert naive[-1] == 2.0 ** 23 + 2 and want[-1] == 2.0 ** 23 + 1
    assert np.any((want != 0) & (np.abs(want) < 2.0 ** -126)) and np.count_nonzero(want[:n // 2] != 0) > n // 4
    # signs of zero and the specials, as IEEE 754 has them
    z = np.float32(0)
    assert not np.signbit(policy.fma32(z, z, -z)) and np.signbit(policy.fma32(-z, z, -z))
    assert not np.signbit(policy.fma32(np.float32(2), np.float32(3), np.float32(-6)))
    assert np.isnan(policy.fma32(np.float32(np.inf), z, z)) and policy.fma32(np.float32(np.inf), np.float32(1), z) == np.inf
    assert policy.fma32(np.float32(3e38), np.float32(2), z) == np.inf and np.isnan(policy.fma32(np.float32(np.nan), z, z))


# ---- the packer ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(4))
def test_packer_round_trips(i):
    net = cases.recorded(i)[0]
    image = policy.pack(net)
    assert image.ctypes.data % 16 == 0 and image.nbytes == _lib_policy.lib().bmpc_policy_packed_bytes(*net.dims)
    layers = policy.unpack(net.dims, image)
    assert len(layers) == net.n_layers + 1
    for l, (W, b, s, t) in enumerate(layers):
        N, K = net.W[l].shape
        assert W.shape == (policy.pad(N), policy.pad(K)) and same_bits(W[:N, :K], net.W[l]) and same_bits(b[:N], net.b[l])
        assert not W[N:].any() and not W[:, K:].any() and not b[N:].any() and not np.signbit(W[N:]).any() and not np.signbit(W[:, K:]).any()
        if net.batch_norm and l < net.n_layers:
            ws, wt = net.scale_shift(l)
            assert same_bits(s[:N], ws) and same_bits(t[:N], wt) and not s[N:].any() and not t[N:].any()
        else:
            assert s is None and t is None
    with pytest.raises(ValueError):
        policy.unpack(net.dims, image[:-16])


def test_constructors_agree():
    import torch
    net, x, _ = cases.recorded(3)
    layers = []
    for l in range(net.n_layers):
        lin, bn = torch.nn.Linear(*net.W[l].shape[::-1]), torch.nn.BatchNorm1d(net.n_hidden, eps=net.eps)
        lin.load_state_dict(dict(weight=torch.from_numpy(net.W[l]), bias=torch.from_numpy(net.b[l])))
        bn.load_state_dict(dict(weight=torch.from_numpy(net.bn[l][0]), bias=torch.from_numpy(net.bn[l][1]), running_mean=torch.from_numpy(net.bn[l][2]),
                                running_var=torch.from_numpy(net.bn[l][3]), num_batches_tracked=torch.tensor(0)))
        layers += [lin, bn, torch.nn.ReLU()]
    out = torch.nn.Linear(net.n_hidden, net.n_out)
    out.load_state_dict(dict(weight=torch.from_numpy(net.W[-1]), bias=torch.from_numpy(net.b[-1])))
    module = torch.nn.Module()
    module.net = torch.nn.Sequential(*layers, out)
    with pytest.raises(ValueError):
        policy.PolicyNet.from_module(module)      # training mode with BatchNorm1d
    other = policy.PolicyNet.from_module(module.eval())
    assert other.dims == net.dims and other.eps == net.eps and same_bits(policy.pack(other), policy.pack(net))
    with pytest.raises(ValueError):
        policy.PolicyNet.from_state_dict({"encoder.weight": np.zeros((3, 3))})


# ---- the twin against the recording ---------------------------------------------------------------------------------------------------------

def _y64(net, x):
    """the network in float64 on the float32-rounded input and the float32 arrays"""
    a = np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    for l in range(net.n_layers + 1):
        a = a @ net.W[l].astype(np.float64).T + net.b[l].astype(np.float64)
        if l < net.n_layers:
            if net.batch_norm:
                gamma, beta, mean, var = (v.astype(np.float64) for v in net.bn[l])
                a = (a - mean) / np.sqrt(var + net.eps) * gamma + beta
            a = np.maximum(a, 0.0)
    return a


@pytest.mark.parametrize("i", range(4))
def test_twin_against_the_recorded_forward(i):
    """max |twin - y64| <= 8 max(max |y_ref - y64|, 2^-24 max |y64|): the twin's sequential chain is as close to the float64 result as
    torch's blocked sums are, within the factor the issue derives (three times the worst ratio seen on five nets, as a power of two)"""
    net, x, y_ref = cases.recorded(i)
    twin, y64 = policy.host_forward(net, x), _y64(net, x)
    assert twin.shape == y_ref.shape == (16, net.n_out) and twin.dtype == np.float32
    e_twin, e_ref = np.abs(twin - y64).max(), np.abs(y_ref - y64).max()
    floor = 2.0 ** -24 * np.abs(y64).max()
    print("net %d %s: twin %.3e, reference %.3e from float64 at outputs up to %.3g: ratio %.2f" % (i, net.dims, e_twin, e_ref, np.abs(y64).max(), e_twin / max(e_ref, floor)))
    assert e_twin <= 8 * max(e_ref, floor)
    assert np.all(np.isfinite(twin))


def test_front_end_equals_the_recording_bit_for_bit():
    r = cases.recording()
    net = cases.recorded(1)[0]
    mean, std = np.concatenate((r["fe_norm0"], r["fe_norm2"])), np.concatenate((r["fe_norm1"], r["fe_norm3"]))
    got = policy.host_input(net, state=r["fe_state"], goal=r["fe_goal"], mean=mean, std=std)
    assert same_bits(got, r["fe_input32"])
    y64 = _y64(net, r["fe_input32"])
    e_twin, e_ref = np.abs(policy.host_layers(net, got) - y64).max(), np.abs(r["fe_y"] - y64).max()
    assert e_twin <= 8 * max(e_ref, 2.0 ** -24 * np.abs(y64).max())


# ---- teeth: a forward pass with one fault fails the bitwise comparison the GPU tests apply --------------------------------------------------

def _restated(net, a, descending=False, no_relu=None, no_bias=None):
    """host_layers again, with room for a fault"""
    for l in range(net.n_layers + 1):
        W, K = net.W[l], net.W[l].shape[1]
        acc = np.broadcast_to(np.float32(0) if l == no_bias else net.b[l], (a.shape[0], W.shape[0])).astype(np.float32)
        ks = range(policy.pad(K))
        for k in (reversed(ks) if descending else ks):
            acc = policy.fma32(W[:, k], a[:, k:k + 1], acc) if k < K else policy.fma32(np.float32(0), np.float32(0), acc)
        if l < net.n_layers:
            if net.batch_norm:
                acc = policy.fma32(acc, *net.scale_shift(l))
            if l != no_relu:
                acc = np.where(acc <= 0, np.float32(0), acc)
        a = acc
    return a


def _variant(net, **kw):
    W, b, bn = [w.copy() for w in net.W], [v.copy() for v in net.b], None if net.bn is None else [tuple(v.copy() for v in g) for g in net.bn]
    kw["edit"](W, b, bn)
    return policy.PolicyNet.from_arrays(W, b, bn, net.eps)


def test_planted_faults_break_the_bitwise_comparison():
    net, x, _ = cases.recorded(0)
    a = policy.host_input(net, x)
    good = policy.host_layers(net, a)
    assert same_bits(_restated(net, a), good)                                   # the restatement is one
    assert not same_bits(_restated(net, a, no_bias=2), good)                    # a bias dropped in one layer
    assert not same_bits(_restated(net, a, no_relu=1), good)                    # ReLU missing on one layer
    assert not same_bits(_restated(net, a, descending=True), good)              # k taken descending

    def transpose(W, b, bn):
        W[1] = np.ascontiguousarray(W[1].T)

    # (a weight of the output layer whose input is live in every row: the widest of the last hidden layer's activations)
    live = int(np.argmax(policy.host_layers(policy.PolicyNet.from_arrays(net.W[:-1], net.b[:-1]), a).min(axis=0)))

    def one_ulp(W, b, bn):
        W[-1][5, live] = np.nextafter(W[-1][5, live], np.float32(np.inf))
    assert not same_bits(policy.host_layers(_variant(net, edit=transpose), a), good)      # W transposed in a square layer
    assert not same_bits(policy.host_layers(_variant(net, edit=one_ulp), a), good)        # one weight moved by one float32 ulp
    # normalisation skipped
    r = cases.recording()
    net1 = cases.recorded(1)[0]
    mean, std = np.concatenate((r["fe_norm0"], r["fe_norm2"])), np.concatenate((r["fe_norm1"], r["fe_norm3"]))
    assert not same_bits(policy.host_forward(net1, state=r["fe_state"], goal=r["fe_goal"]),
                         policy.host_forward(net1, state=r["fe_state"], goal=r["fe_goal"], mean=mean, std=std))
    # BatchNorm's t without running_mean
    net3, x3, _ = cases.recorded(3)

    def no_mean(W, b, bn):
        bn[0][2][:] = 0
    assert not same_bits(policy.host_forward(_variant(net3, edit=no_mean), x3), policy.host_forward(net3, x3))
    assert same_bits(_restated(net3, policy.host_input(net3, x3)), policy.host_forward(net3, x3))
