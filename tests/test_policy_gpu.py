"""include/ext/bunmpc_policy.h on the GPU, through bunmpc_amd/policy.py::DevicePolicy and the C-ABI: every output equals the numpy twin
(bunmpc_amd/policy.py::host_forward, host_tau, host_l1_rows) in every bit -- which is also the check that gfx950's fp32 matrix cores
compute the k-ascending fmaf chain the header states."""
import ctypes as C
import functools

import numpy as np
import pytest

from bunmpc_amd import policy
from tests import dataset_np
from tests import policy_cases as cases
from tests.policy_cases import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a):
    import torch
    return torch.as_tensor(np.array(a, dtype=np.float64), device=DEV)


@functools.lru_cache(maxsize=None)
def _policy(which):
    net = cases.wide_net() if which == "wide" else cases.recorded(which)[0]
    return policy.DevicePolicy(net, DEV)


def _wide64(a):
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _wide_case():
    """2 tile + 3 rows for the 256-wide net and the twin's result: rows do not depend on one another, so every smaller n is a prefix"""
    tile = _policy("wide").tile
    x = np.random.default_rng(7).normal(size=(2 * tile + 3, cases.WIDE[0]))
    return cases.frozen(x), cases.frozen(policy.host_forward(cases.wide_net(), x))


@pytest.mark.parametrize("i", range(4))
def test_recorded_nets_equal_the_twin(i):
    net, x, _ = cases.recorded(i)
    assert i < cases.n_recorded()
    got = _policy(i).forward(_dev(x)).cpu().numpy()
    want = _wide64(policy.host_forward(net, x))
    assert same_bits(got, want), np.argwhere(got != want)[:4]
    assert np.all(x[8] != 0) and np.all(np.abs(x[8].astype(np.float32)) < 2.0 ** -126)      # the subnormal row went in as subnormals


def test_wide_net_at_the_tile_boundaries():
    dp = _policy("wide")
    x, want = _wide_case()
    tile = dp.tile
    assert x.shape[0] == 2 * tile + 3
    outs = [(n, dp.forward(_dev(x[:n]))) for n in (1, tile - 1, tile, tile + 1, 2 * tile + 3)]
    for n, got in outs:
        assert same_bits(got.cpu().numpy(), _wide64(want[:n])), n


def _raw(dp, n, **fields):
    r = policy._lib_policy.PolicyRows()
    r.n = n
    for k, v in fields.items():
        setattr(r, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    import torch
    policy._lib.check(policy._lib_policy.lib().bmpc_policy_forward_device(C.byref(dp.desc), C.byref(r), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def test_outputs_past_n_are_untouched():
    import torch
    dp = _policy(0)
    net, x, _ = cases.recorded(0)
    n, guard = 13, -12345.678
    q, v, label = np.random.default_rng(3).normal(size=(16, 19)), np.random.default_rng(4).normal(size=(16, 18)), np.random.default_rng(5).normal(size=(16, 12))
    action, tau, err = (torch.full(s, guard, dtype=torch.float64, device=DEV) for s in ((16, 12), (16, 12), (16,)))
    _raw(dp, n, x=_dev(x), x_stride=48, action=action, tau=tau, action_type=policy._lib_policy.ACTION_TYPE["pd_target"], q=_dev(q), q_stride=19,
         v=_dev(v), v_stride=18, kp=2.0, kd=0.1, err=err, label=_dev(label), label_stride=12)
    y = policy.host_forward(net, x)
    for got, want in ((action, _wide64(y)), (tau, policy.host_tau(y, q, v, 2.0, 0.1, "pd_target")), (err, policy.host_l1_rows(y, label))):
        got = got.cpu().numpy()
        assert same_bits(got[:n], want[:n]) and np.all(got[n:] == guard)
    _raw(dp, 0, x=_dev(x), x_stride=48, action=action)      # n = 0: nothing runs
    assert same_bits(action.cpu().numpy()[:n], _wide64(y)[:n])


@pytest.mark.parametrize("norm", [False, True])
def test_both_input_forms_in_place(norm):
    """state and goal as views of one (n, 60) buffer (stride 60), against the assembled x; with and without mean / std"""
    rng = np.random.default_rng(11)
    net, _, _ = cases.recorded(1)
    dp = _policy(1)
    buf = rng.normal(size=(37, 60)) * 3.0
    state, goal = buf[:, 2:45], buf[:, 47:59]
    mean, std = rng.normal(size=55), rng.uniform(0.05, 3.0, size=55)
    d = _dev(buf)
    action, tau = dp.act(d[:, 2:45], d[:, 47:59], norm=(_dev(mean), _dev(std)) if norm else None, action_type="torque")
    want = policy.host_forward(net, state=state, goal=goal, mean=mean if norm else None, std=std if norm else None)
    assert same_bits(action.cpu().numpy(), _wide64(want)) and same_bits(tau.cpu().numpy(), _wide64(want))
    with np.errstate(all="ignore"):
        x = (np.hstack((state, goal)) - mean) / std if norm else np.hstack((state, goal))
    assert same_bits(dp.forward(_dev(x)).cpu().numpy(), _wide64(want))


def test_front_end_of_the_recording():
    r = cases.recording()
    dp = _policy(1)
    norm = (_dev(np.concatenate((r["fe_norm0"], r["fe_norm2"]))), _dev(np.concatenate((r["fe_norm1"], r["fe_norm3"]))))
    action, _ = dp.act(_dev(r["fe_state"]), _dev(r["fe_goal"]), norm=norm)
    assert same_bits(action.cpu().numpy(), _wide64(policy.host_layers(cases.recorded(1)[0], r["fe_input32"])))


def test_input_that_is_only_8_byte_aligned():
    import torch
    net, x, _ = cases.recorded(1)      # rows of 55 doubles: every other row starts 8 bytes off anyway; here the first does
    flat = torch.empty(x.size + 1, dtype=torch.float64, device=DEV)
    flat[1:].copy_(torch.from_numpy(x.reshape(-1)))
    view = flat[1:].view(x.shape)
    assert view.data_ptr() % 16 == 8
    assert same_bits(_policy(1).forward(view).cpu().numpy(), _wide64(policy.host_forward(net, x)))


def test_a_non_finite_row_stays_alone():
    x, want = _wide_case()
    x = x[:40].copy()
    x[5, 3], x[17], x[33, 54] = np.nan, np.inf, -np.inf
    got = _policy("wide").forward(_dev(x)).cpu().numpy()
    bad = np.zeros(40, bool)
    bad[[5, 17, 33]] = True
    assert np.all(np.isnan(got[bad])) and same_bits(got[~bad], _wide64(want[:40][~bad]))
    assert same_bits(got, _wide64(policy.host_forward(cases.wide_net(), x)))


def _subnormal_case():
    """a net whose first layer works in the subnormal range throughout -- weights, biases, products, sums, activations -- and whose
    later layers bring that back to sizes at which it decides the output's bits; inputs partly subnormal too"""
    rng = np.random.default_rng(13)
    net = cases.random_net(rng, 55, 72, 2, 12)
    net.W[0] *= np.float32(1e-39)
    net.b[0] *= np.float32(1e-39)
    net.W[1] *= np.float32(1e31)
    net.b[1] *= np.float32(1e-8)
    net.b[2] *= np.float32(1e-8)
    x = rng.normal(size=(35, 55))
    x[1] *= 1e-42
    x[2, ::2] *= 1e-40
    want = policy.host_forward(net, x)
    tiny = lambda a: (a != 0) & (np.abs(a) < 2.0 ** -126)      # noqa: E731
    first = policy.host_layers(policy.PolicyNet.from_arrays([net.W[0], np.eye(72)], [net.b[0], np.zeros(72)]), policy.host_input(net, x))
    assert np.all(tiny(net.W[0])) and np.all(tiny(net.b[0])) and np.any(tiny(policy.host_input(net, x))) and np.all(tiny(first) | (first == 0)) and np.any(first != 0)
    flushed = policy.PolicyNet.from_arrays([0 * net.W[0]] + net.W[1:], [0 * net.b[0]] + net.b[1:])      # what flushing to zero would compute
    assert np.all(np.isfinite(want)) and np.all(want != policy.host_forward(flushed, x))
    return net, x, want


def test_subnormal_inputs_and_weights():
    net, x, want = _subnormal_case()
    assert same_bits(policy.DevicePolicy(net, DEV).forward(_dev(x)).cpu().numpy(), _wide64(want))


@pytest.mark.parametrize("action_type,which", [("torque", 0), ("pd_target", 0), ("structured", 2)])
def test_tau_from_a_q_v_buffer_in_place(action_type, which):
    rng = np.random.default_rng(17)
    net, x, _ = cases.recorded(which)
    qv = rng.normal(size=(16, 37))
    d = _dev(qv)
    action, tau = _policy(which).act(_dev(x[:, :43]), _dev(x[:, 43:]), q=d[:, :19], v=d[:, 19:], kp=2.5, kd=0.15, action_type=action_type)
    y = policy.host_forward(net, x)
    assert same_bits(action.cpu().numpy(), _wide64(y))
    assert same_bits(tau.cpu().numpy(), policy.host_tau(y, qv[:, :19], qv[:, 19:], 2.5, 0.15, action_type))


def test_two_calls_on_one_stream_one_read_back():
    import torch
    dp = _policy(0)
    net, x, _ = cases.recorded(0)
    first = dp.forward(_dev(x))
    second = dp.forward(torch.cat((first, first, first, first), dim=1))      # the first call's result is the second call's input
    y1 = _wide64(policy.host_forward(net, x))
    got = torch.cat((first, second), dim=1).cpu().numpy()
    assert same_bits(got, np.hstack((y1, _wide64(policy.host_forward(net, np.hstack((y1, y1, y1, y1)))))))


def test_l1_rows_over_a_device_data_set():
    """DeviceDatabase.batch(index) -> l1_rows, against the twin network fed the twin data set's rows (normalised with the statistics
    the device computed, which the data set's own tests hold to numpy's)"""
    from bunmpc_amd.dataset_device import DeviceDatabase
    rng = np.random.default_rng(19)
    g = dict(states=rng.normal(size=(90, 43)) * 2.0 + 1.0, actions=rng.normal(size=(90, 12)), vc_goals=rng.normal(size=(90, 5)), cc_goals=rng.normal(size=(90, 12)))
    db, tw = DeviceDatabase(100, goal_horizon=1, device=DEV, max_problems=256), dataset_np.TwinDatabase(100, w_cc=12)
    db.append(**{k: _dev(v) for k, v in g.items()})
    tw.append(**g)
    db.calc_input_mean_std()
    mean, std = policy.DevicePolicy.norm_of(db)
    index = rng.integers(0, 90, size=70)
    x, y = db.batch(index)
    dp = _policy(1)
    err = dp.l1_rows(x, y)
    in_place, _ = dp.act(db.states[:90], db.cc_goals[:90], norm=(mean, std))      # the ring's rows, normalised by the kernel itself
    stats = {"states": (mean[:43].cpu().numpy(), std[:43].cpu().numpy()), "cc_goals": (mean[43:].cpu().numpy(), std[43:].cpu().numpy())}
    tx, ty = tw.batch(index, stats=stats)
    net = cases.recorded(1)[0]
    assert same_bits(err.cpu().numpy(), policy.host_l1_rows(policy.host_forward(net, tx), ty))
    assert same_bits(in_place.cpu().numpy()[index], _wide64(policy.host_forward(net, tx)))
