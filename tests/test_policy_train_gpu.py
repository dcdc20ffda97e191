"""include/ext/bunmpc_policy_train.h on the GPU, through bunmpc_amd/policy_train.py::DeviceTrainer and the C-ABI: the loss, every
gradient, every parameter, Adam's moments and the running statistics equal the numpy twin (host_step) in every bit, one step and five;
the packed image written on the device equals the host packer's; and fit on a DeviceDatabase equals the twin's loop."""
import ctypes as C

import numpy as np
import pytest

from bunmpc_amd import _lib_policy_train, policy
from bunmpc_amd import policy_train as pt
from tests import dataset_np, policy_cases
from tests import policy_train_cases as cases
from tests.policy_train_cases import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = -12345.678


def _dev(a):
    import torch
    return torch.as_tensor(np.array(a, dtype=np.float64), device=DEV)


def _trainer(state, t=0, lr=0.002):
    """a DeviceTrainer started from a TrainState: the moments and the count go up too"""
    import torch
    trainer = pt.DeviceTrainer(state.net(), DEV, lr=lr, keep_grads=True)
    for mine, theirs in ((trainer.m, state.m), (trainer.v, state.v)):
        for (_, a), (_, b) in zip(mine.arrays(), theirs.arrays()):
            a.copy_(torch.from_numpy(np.array(b)))
    trainer.t = t
    return trainer


def _grads(trainer):
    return trainer.grads().map(lambda a: a.cpu().numpy())


def _one_step(state, x, y, lr=0.002, t=1):
    """the device's step and the twin's from `state`: the name of the first array that differs, or None"""
    trainer = _trainer(state, t - 1, lr)
    loss = trainer.step(_dev(x), _dev(y))
    want, want_loss, want_g = pt.host_step(state, x, y, lr, t)
    if not same_bits(loss.cpu().numpy(), np.float64(want_loss)):
        return "loss: %r for %r" % (float(loss), float(want_loss))
    return cases.first_difference(trainer.state(), want, _grads(trainer), want_g)


@pytest.mark.parametrize("i,k", [(0, 0), (1, 0), (2, 0), (0, 1000), (2, 2)])
def test_one_step_on_the_recorded_nets_equals_the_twin(i, k):
    c = cases.recorded(i, k)
    trainer = _trainer(c["before"], c["t"] - 1, c["lr"])
    loss = trainer.step(_dev(c["x"]), _dev(c["y"]))
    want, want_loss, want_g, _ = cases.twin_step(i, k)
    assert same_bits(loss.cpu().numpy(), np.float64(want_loss))
    assert cases.first_difference(trainer.state(), want, _grads(trainer), want_g) is None


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33])
def test_small_batches_equal_the_twin(n):
    tile = _lib_policy_train.lib().bmpc_policy_train_tile()
    assert n < tile
    net, x, y = cases.drawn(100 + n, 23, 24, 2, 12, n > 1, n)      # one row is a batch without BatchNorm only
    assert _one_step(pt.TrainState.from_net(net), x, y) is None


@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_row_tile_boundaries_equal_the_twin(offset):
    n = _lib_policy_train.lib().bmpc_policy_train_tile() + offset
    net, x, y = cases.drawn(200 + offset, 23, 24, 2, 12, True, n)
    assert _one_step(pt.TrainState.from_net(net), x, y) is None


@pytest.mark.parametrize("n", [48, 256])
def test_width_256_equals_the_twin(n):
    """(55, 256, 2, 12, BatchNorm): 16 x 16 tiles of dW in 16 rows and columns, the output layer's 12 columns in a tile of 16; n = 256 is
    the reference's batch"""
    net, x, y = cases.drawn(300 + n, 55, 256, 2, 12, True, n)
    assert _one_step(pt.TrainState.from_net(net), x, y) is None


@pytest.mark.parametrize("dims", [(23, 48, 2, 36, 0), (55, 40, 3, 12, 1)])
def test_five_consecutive_steps_with_a_changing_rate_equal_the_twin(dims):
    net, _, _ = cases.drawn(400 + dims[1], *dims, 1)
    rng = np.random.default_rng(401)
    state, trainer = pt.TrainState.from_net(net), pt.DeviceTrainer(net, DEV, keep_grads=True)
    losses, want_losses = [], []
    for t, lr in enumerate((0.002, 0.002, 0.01, 0.0005, 0.003), start=1):
        x, y = rng.normal(size=(40, dims[0])), rng.normal(size=(40, dims[3]))
        losses.append(trainer.step(_dev(x), _dev(y), lr=lr))
        state, loss, g = pt.host_step(state, x, y, lr, t)
        want_losses.append(loss)
    import torch
    assert same_bits(torch.stack(losses).cpu().numpy(), np.array(want_losses, np.float64))
    assert cases.first_difference(trainer.state(), state, _grads(trainer), g) is None and trainer.t == 5


def test_a_subnormal_first_layer_is_kept_forward_and_backward():
    """the first layer works in the subnormal range throughout (tests/test_policy_gpu.py::_subnormal_case): its activations go forward
    as subnormals, and the next layer's gradient dW_1 = dz_1' a_1 is a chain of subnormal products with subnormal sums (flushing any
    of them would leave it zero); half the input columns are subnormal too"""
    rng = np.random.default_rng(13)
    net = policy_cases.random_net(rng, 55, 72, 2, 12)
    net.W[0] *= np.float32(1e-39)
    net.b[0] *= np.float32(1e-39)
    net.W[1] *= np.float32(1e31)
    net.b[1] *= np.float32(1e-8)
    net.b[2] *= np.float32(1e-8)
    x, y = rng.normal(size=(35, 55)), rng.normal(size=(35, 12))
    x[:, ::2] *= 1e-38
    state = pt.TrainState.from_net(net)
    fwd = pt.host_train_forward(state, x)
    tiny = lambda a: (a != 0) & (np.abs(a) < 2.0 ** -126)      # noqa: E731
    g = pt.host_backward(state, fwd, y)
    assert np.all(tiny(fwd["a"][1]) | (fwd["a"][1] == 0)) and np.any(tiny(fwd["a"][1])) and np.all(np.isfinite(fwd["p"]))
    assert np.all(tiny(g.W[1]) | (g.W[1] == 0)) and np.count_nonzero(g.W[1]) > g.W[1].size // 4 and np.any(tiny(policy.host_input(net, x)))
    flushed = pt.TrainState.from_net(policy.PolicyNet.from_arrays([0 * net.W[0]] + net.W[1:], [0 * net.b[0]] + net.b[1:]))
    assert not same_bits(pt.host_train_forward(flushed, x)["p"], fwd["p"])      # what flushing to zero would compute
    assert _one_step(state, x, y) is None


@pytest.mark.parametrize("bn", [False, True])
def test_packed_image_on_the_device_equals_the_host_packer_s(bn):
    net, x, y = cases.drawn(500 + bn, 55, 40, 3, 12, bn, 40)
    trainer = pt.DeviceTrainer(net, DEV)
    dp = trainer.policy      # held across the step: the step rewrites its image
    before = dp.packed.cpu().numpy()
    assert same_bits(before, policy.pack(net))
    trainer.step(_dev(x), _dev(y))
    assert trainer.policy is dp
    trained = trainer.net()
    image = dp.packed.cpu().numpy()
    assert same_bits(image, policy.pack(trained)) and not same_bits(image, before)
    assert same_bits(dp.forward(_dev(x)).cpu().numpy(), policy.host_forward(trained, x).astype(np.float64))
    assert same_bits(trainer.l1_rows(_dev(x), _dev(y)).cpu().numpy(), policy.host_l1_rows(policy.host_forward(trained, x), y))
    sd = trainer.state_dict()
    assert [k for k in sd if k.endswith("num_batches_tracked")] == (["net.1.num_batches_tracked", "net.4.num_batches_tracked", "net.7.num_batches_tracked"] if bn else [])
    assert same_bits(sd["net.0.weight"].cpu().numpy(), trained.W[0]) and all(int(v) == 1 for k, v in sd.items() if k.endswith("tracked"))


def test_inputs_in_place_guards_and_two_streams():
    import torch
    net, x, y = cases.drawn(600, 23, 24, 2, 12, True, 37)
    state = pt.TrainState.from_net(net)
    want, want_loss, want_g = pt.host_step(state, x, y, 0.002, 1)
    # x and y as strided views of one buffer whose first row starts 8 bytes off a 16-byte boundary
    flat = torch.full((37 * 40 + 1,), GUARD, dtype=torch.float64, device=DEV)
    buf = flat[1:].view(37, 40)
    buf[:, 2:25], buf[:, 27:39] = _dev(x), _dev(y)
    assert buf.data_ptr() % 16 == 8
    # the loss goes into the middle of a guarded vector; a second trainer on a second stream takes the rows in the other order
    trainer = pt.DeviceTrainer(net, DEV, keep_grads=True)
    slots = torch.full((3,), GUARD, dtype=torch.float64, device=DEV)
    other = pt.DeviceTrainer(net, DEV, keep_grads=True)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        trainer.step(buf[:, 2:25], buf[:, 27:39], out=slots[1:2])
    with torch.cuda.stream(s2):
        x2, y2 = _dev(x[::-1].copy()), _dev(y[::-1].copy())
        loss2 = other.step(x2, y2)
    torch.cuda.synchronize()
    got = slots.cpu().numpy()
    assert got[0] == GUARD and got[2] == GUARD and same_bits(got[1:2], np.array([want_loss]))
    assert cases.first_difference(trainer.state(), want, _grads(trainer), want_g) is None
    left = buf.cpu().numpy()
    assert same_bits(left[:, 2:25], x) and same_bits(left[:, 27:39], y) and np.all(left[:, :2] == GUARD) and np.all(left[:, 25:27] == GUARD) and np.all(left[:, 39:] == GUARD)
    want2, want_loss2, want_g2 = pt.host_step(state, x[::-1], y[::-1], 0.002, 1)
    assert same_bits(loss2.cpu().numpy(), np.float64(want_loss2)) and cases.first_difference(other.state(), want2, _grads(other), want_g2) is None


def test_parameter_arrays_are_written_within_their_bounds():
    """the C-ABI on arrays cut out of one guarded buffer each: every parameter, moment, gradient and running statistic, and the scratch"""
    import torch
    net, x, y = cases.drawn(700, 23, 24, 2, 12, True, 19)
    state = pt.TrainState.from_net(net)
    d = _lib_policy_train.PolicyTrain()
    d.n_in, d.n_hidden, d.n_layers, d.n_out, d.batch_norm = net.dims
    d.eps = net.eps
    grads = _lib_policy_train.PolicyParams()
    held = []

    def guarded(a):
        size = (a.size + 3) // 4 * 4      # (the next array starts 16-byte aligned, 4 guard floats on)
        t = torch.full((size + 8,), GUARD, dtype=torch.float32, device=DEV)
        t[4:4 + a.size] = torch.from_numpy(np.array(a, np.float32).reshape(-1))
        held.append((t, a.size))
        return t[4:].data_ptr()

    for q, desc in ((state.p, d.p), (state.m, d.m), (state.v, d.v), (state.p, grads)):
        for l in range(3):
            desc.W[l], desc.b[l] = guarded(q.W[l]), guarded(q.b[l])
        for l in range(2):
            desc.gamma[l], desc.beta[l] = guarded(q.gamma[l]), guarded(q.beta[l])
    for l in range(2):
        d.running_mean[l], d.running_var[l] = guarded(state.running_mean[l]), guarded(state.running_var[l])
    need = _lib_policy_train.lib().bmpc_policy_train_work_bytes(*net.dims, 19)
    d.work, d.work_bytes = guarded(np.zeros(need // 4)), need
    s = _lib_policy_train.PolicyStep()
    xd, yd, loss = _dev(x), _dev(y), torch.zeros((), dtype=torch.float64, device=DEV)
    s.n, s.x, s.x_stride, s.y, s.y_stride, s.loss, s.lr, s.grads = 19, xd.data_ptr(), 23, yd.data_ptr(), 12, loss.data_ptr(), 0.002, C.addressof(grads)
    s.bc1, s.bc2 = pt.bias_corrections(1)
    policy._lib.check(_lib_policy_train.lib().bmpc_policy_train_step_device(C.byref(d), C.byref(s), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    image = torch.full((policy.pack(net).size + 8,), GUARD, dtype=torch.float32, device=DEV)
    policy._lib.check(_lib_policy_train.lib().bmpc_policy_pack_device(C.byref(d), C.c_void_p(image[4:].data_ptr()), 4 * (image.numel() - 8), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    want, want_loss, want_g = pt.host_step(state, x, y, 0.002, 1)
    assert same_bits(loss.cpu().numpy(), np.float64(want_loss))
    order = lambda q: [a for l in range(3) for a in (q.W[l], q.b[l])] + [a for l in range(2) for a in (q.gamma[l], q.beta[l])]      # noqa: E731
    wanted = [a for q in (want.p, want.m, want.v, want_g) for a in order(q)] + [a for l in range(2) for a in (want.running_mean[l], want.running_var[l])]
    assert len(wanted) == len(held) - 1
    for (t, size), a in zip(held, wanted + [None]):
        got = t.cpu().numpy()
        assert np.all(got[:4] == np.float32(GUARD)) and np.all(got[4 + size:] == np.float32(GUARD))
        if a is not None:
            assert same_bits(got[4:4 + size], np.asarray(a).reshape(-1))
    got = image.cpu().numpy()
    assert np.all(got[:4] == np.float32(GUARD)) and np.all(got[-4:] == np.float32(GUARD)) and same_bits(got[4:-4], policy.pack(want.net()))


def test_fit_on_a_device_data_set_equals_the_twin_s_loop():
    from bunmpc_amd.dataset_device import DeviceDatabase
    rng = np.random.default_rng(23)
    g = dict(states=rng.normal(size=(600, 43)), actions=rng.normal(size=(600, 12)), vc_goals=rng.normal(size=(600, 5)), cc_goals=rng.normal(size=(600, 12)))
    db, tw = DeviceDatabase(640, goal_horizon=1, device=DEV, norm_input=False, max_problems=1024), dataset_np.TwinDatabase(640, w_cc=12)
    db.append(**{k: _dev(v) for k, v in g.items()})
    tw.append(**g)

    class Rows:
        def __len__(self):
            return tw.length

        def batch(self, index):
            return tw.batch(index, normalise=False)

    net = policy_cases.random_net(np.random.default_rng(24), 55, 32, 2, 12, True)
    trainer, twin = pt.DeviceTrainer(net, DEV, lr=0.002), pt.HostTrainer(net, lr=0.002)
    history = trainer.fit(db, n_epoch=2, batch_size=64, n_train_frac=0.9, seed=3)
    want = twin.fit(Rows(), n_epoch=2, batch_size=64, n_train_frac=0.9, seed=3)
    assert len(history) == 2 and trainer.t == twin.t == 16
    assert same_bits(np.array(history), np.array(want)) and np.all(np.isfinite(np.array(history)))
    assert cases.first_difference(trainer.state(), twin.state) is None
    assert same_bits(trainer.policy.packed.cpu().numpy(), policy.pack(twin.net()))
