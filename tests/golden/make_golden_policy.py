"""Record tests/golden/policy/policy_ref.npz: weights, inputs and the float32 outputs of the REFERENCE's own policy network.

Run by hand, on a machine that has the reference beside this repository, with torch on the CPU:

    python tests/golden/make_golden_policy.py <path of iterative_supervised_learning> [--out tests/golden/policy/policy_ref.npz]

It loads examples/iterative_algorithm/networks.py from its place and builds GoalConditionedPolicyNet as the trainers do.  Its
initialisation leaves every bias zero, so the biases are redrawn; the BatchNorm1d net gets running statistics and affine terms away
from (0, 1, 1, 0) and is put in eval().  Only arrays go into the file; no test reads the reference.

Per net `n<i>_`: dims (in, hidden, hidden layers, out, batch_norm), eps, keys (the state_dict's keys, in order) and sd<j> (their arrays),
x (16, in) float64 -- N(0, 1); rows 4-7 scaled by 1e3; row 8 holds float32 subnormals; row 9 is exact zeros -- and y (16, out) float32 =
net(torch.from_numpy(x).float()).  `fe_`: the front end of simulation.py:1702-1710 on one row of net 1: state (1, 43), goal (1, 12),
norm0..3 = [state_mean, state_std, goal_mean, goal_std], input32 = torch.from_numpy(np.hstack(...)).float(), y = net 1 of it."""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NETS = [(48, 64, 4, 12, False), (55, 72, 2, 12, False), (67, 32, 1, 36, False), (55, 64, 3, 12, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("isl")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "policy", "policy_ref.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("networks", os.path.join(args.isl, "examples", "iterative_algorithm", "networks.py"))
    networks = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(networks)
    torch.manual_seed(20240607)
    rng = np.random.default_rng(20240607)
    out, nets = {}, []
    for i, (n_in, hidden, layers, n_out, bn) in enumerate(NETS):
        net = networks.GoalConditionedPolicyNet(n_in, n_out, num_hidden_layer=layers, hidden_dim=hidden, batch_norm=bn)
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.Linear):
                    m.bias.normal_(0.0, 0.2)
                elif isinstance(m, torch.nn.BatchNorm1d):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.normal_(0.0, 0.3)
                    m.running_mean.normal_(0.0, 0.5)
                    m.running_var.uniform_(0.3, 2.5)
        net.eval()
        x = rng.normal(size=(16, n_in))
        x[4:8] *= 1e3
        x[8] = rng.normal(size=n_in) * 1e-40
        x[9] = 0.0
        with torch.no_grad():
            y = net(torch.from_numpy(x).float()).numpy()
        sd = net.state_dict()
        k = "n%d_" % i
        out[k + "dims"] = np.array([n_in, hidden, layers, n_out, int(bn)])
        out[k + "eps"] = np.array(next((m.eps for m in net.modules() if isinstance(m, torch.nn.BatchNorm1d)), 1e-5))
        out[k + "keys"] = np.array(list(sd.keys()))
        for j, v in enumerate(sd.values()):
            out[k + "sd%d" % j] = v.numpy()
        out[k + "x"], out[k + "y"] = x, y
        nets.append(net)
    # the front end of simulation.py:1702-1710, as written there
    state, goal = rng.normal(size=(1, 43)) * 3.0 + 0.5, rng.normal(size=(1, 12))
    norm_policy_input = [rng.normal(size=43), rng.uniform(0.05, 4.0, size=43), rng.normal(size=12) * 0.2, rng.uniform(0.05, 2.0, size=12)]
    out["fe_state"], out["fe_goal"] = state, goal
    for j, v in enumerate(norm_policy_input):
        out["fe_norm%d" % j] = v
    state = (state - norm_policy_input[0]) / norm_policy_input[1]
    goal = (goal - norm_policy_input[2]) / norm_policy_input[3]
    input = np.hstack((state, goal))
    x32 = torch.from_numpy(input).float()
    out["fe_input32"] = x32.numpy()
    with torch.no_grad():
        out["fe_y"] = nets[1](x32).numpy()
    out["n_nets"] = np.asarray(len(NETS))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("%d nets -> %s (%d bytes)" % (len(NETS), args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
