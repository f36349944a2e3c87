"""CPU (-m "not gpu"): the sampled-tape family on the host (the ABI of include/envbuild_sample.h: tests/test_family_abi.py): the NumPy / torch
restatement of the noise and the samples (env_build_amd/sample.py) has the moments, the AR(1) correlation, the repeatability and the
env-id keying the header states; SamplingMPC's loop (mpc.sampling_loop) is elitist on a non-convex toy cost."""
import math

import numpy as np
import pytest


# ---- the restatement of the noise and the samples ----
def test_noise_moments_over_2_to_the_20_draws():
    from env_build_amd.sample import sample_noise_reference
    S, H, B = 129, 128, 32                                  # 128 noisy samples x 128 steps x 32 envs x 2 components = 2^20 draws
    eps = sample_noise_reference(np.arange(B), S, H, seed=11, counter=3, beta=0.0)
    assert eps.dtype == np.float32 and eps.shape == (S, H, B, 2) and not eps[0].any()
    x = eps[1:].astype(np.float64).ravel()
    n = x.size
    assert n == 1 << 20
    print('noise over %d draws: mean %.3e, variance %.6f, min %.3f, max %.3f' % (n, x.mean(), x.var(), x.min(), x.max()))
    assert abs(x.mean()) <= 4.0 / math.sqrt(n)
    assert abs(x.var() - 1.0) <= 0.01
    assert np.abs(x).max() <= 2.0 * 1.7320508 + 1e-6        # a sum of four uniforms


@pytest.mark.parametrize('beta', [0.7, 0.3])
def test_ar1_lag_one_correlation_is_beta(beta):
    from env_build_amd.sample import sample_noise_reference
    eps = sample_noise_reference(np.arange(32), 129, 128, seed=5, counter=0, beta=beta)[1:].astype(np.float64)
    var = eps.var()
    rho = ((eps[:, 1:] * eps[:, :-1]).mean() - eps[:, 1:].mean() * eps[:, :-1].mean()) / var
    print('AR(1) beta %.2f: lag-1 correlation %.4f, variance %.4f' % (beta, rho, var))
    assert abs(rho - beta) <= 0.01 and abs(var - 1.0) <= 0.01           # the gain keeps the variance at 1


def test_samples_repeat_follow_the_counter_and_the_env_id():
    import torch
    from env_build_amd.sample import sample_tapes_reference
    H, B, S = 7, 6, 5
    g = torch.Generator().manual_seed(0)
    nominal = torch.rand((H, B, 2), generator=g) * 2.6 - 1.3              # on and beyond the box
    nominal[2, 1, 0], nominal[3, 1, 1] = 1.0, -1.0
    a = sample_tapes_reference(nominal, S, 9, 4, (0.3, 0.2), beta=0.5)
    b = sample_tapes_reference(nominal, S, 9, 4, (0.3, 0.2), beta=0.5)
    c = sample_tapes_reference(nominal, S, 9, 5, (0.3, 0.2), beta=0.5)
    assert a.shape == (S, H, B, 2) and a.dtype == torch.float32
    assert torch.equal(a, b)                                              # the same (seed, counter): the same bits
    assert torch.equal(a[0], nominal.clamp(-1, 1)) and torch.equal(c[0], a[0])      # sample 0 is the nominal
    free = (a[1:].abs() < 1.0) & (c[1:].abs() < 1.0)                      # neither on the box
    assert int(free.sum()) > free.numel() // 3 and bool((a[1:] != c[1:])[free].all())   # another counter: every draw differs
    assert float(a.abs().max()) <= 1.0
    # a zero sigma leaves that component at the nominal
    z = sample_tapes_reference(nominal, S, 9, 4, (0.3, 0.0), beta=0.5)
    assert torch.equal(z[:, :, :, 1], nominal.clamp(-1, 1)[:, :, 1].expand(S, H, B)) and torch.equal(z[..., 0], a[..., 0])
    # an env's noise follows its id, not its row
    ids = torch.tensor([40, 3, 17, 0, 2 ** 31 - 1, 8])
    perm = torch.tensor([3, 0, 5, 1, 4, 2])
    with_ids = sample_tapes_reference(nominal, S, 9, 4, (0.3, 0.2), 0.5, env_ids=ids)
    permuted = sample_tapes_reference(nominal[:, perm], S, 9, 4, (0.3, 0.2), 0.5, env_ids=ids[perm])
    assert torch.equal(permuted, with_ids[:, :, perm])
    assert torch.equal(sample_tapes_reference(nominal, S, 9, 4, (0.3, 0.2), 0.5, env_ids=torch.arange(B)), a)
    assert not torch.equal(with_ids[1:], a[1:])
    # float64: the float32 noise, the arithmetic of the dtype
    d = sample_tapes_reference(nominal.double(), S, 9, 4, (0.3, 0.2), beta=0.5)
    assert d.dtype == torch.float64 and float((d - a.double()).abs().max()) <= 2.0 ** -23


def test_softmin_mean_reference():
    import torch
    from env_build_amd.sample import softmin_mean_reference
    nan = float('nan')
    S, H, B = 4, 3, 5
    g = torch.Generator().manual_seed(1)
    samples = (torch.rand((S, H, B, 2), generator=g, dtype=torch.float64) * 2 - 1)
    cost = torch.tensor([[3.0, nan, nan, 1.0, float('inf')],
                         [1.0, 2.0, nan, 1.0, nan],
                         [1.0, nan, nan, 5.0, nan],
                         [2.0, 2.5, nan, nan, nan]], dtype=torch.float64)
    mean, idx = softmin_mean_reference(samples, cost, 0.5)
    assert idx.tolist() == [1, 1, 0, 0, 0]
    w = torch.exp(-(cost[:, 0] - 1.0) / 0.5)
    assert torch.allclose(mean[:, 0], (w.view(S, 1, 1) * samples[:, :, 0]).sum(0) / w.sum())
    w = torch.tensor([0.0, 1.0, 0.0, math.exp(-1.0)], dtype=torch.float64)
    assert torch.allclose(mean[:, 1], (w.view(S, 1, 1) * samples[:, :, 1]).sum(0) / w.sum())
    assert torch.equal(mean[:, 2], samples[0, :, 2]) and torch.equal(mean[:, 4], samples[0, :, 4])    # no finite cost: sample 0
    plain, _ = softmin_mean_reference(samples, cost, float('inf'))
    assert torch.allclose(plain[:, 0], samples[:, :, 0].mean(0))
    sharp, _ = softmin_mean_reference(samples, cost, 1e-9)
    assert torch.allclose(sharp[:, 1], samples[1, :, 1])


# ---- SamplingMPC's loop, on the CPU ----
def bumpy_cost(H, B, seed=0):
    """J_b(u) = scale_b (1/2 sum c (u - m_b)^2 + sum_j A_j exp(-|u - p_j|^2 / 0.8)): a bowl whose minimum lies partly outside the box,
    with three bumps (non-convex), envs of very different scale, and a last env whose cost is always NaN"""
    import torch
    g = torch.Generator().manual_seed(seed)
    m = torch.randn((H, B, 2), generator=g) * 1.5
    c = torch.rand((H, 1, 2), generator=g) * 20.0 + 0.05
    scale = torch.logspace(-2, 1, B)
    bumps = [(torch.rand((H, B, 2), generator=g) * 2 - 1, amp) for amp in (25.0, -15.0, 40.0)]

    def cost(U):                                            # [S, H, B, 2] -> [S, B]
        J = (0.5 * c * (U - m) ** 2).sum((1, 3))
        for p, amp in bumps:
            J = J + amp * torch.exp(-((U - p) ** 2).sum((1, 3)) / 0.8)
        J = J * scale
        J[:, B - 1] = float('nan')
        return J
    return cost


def test_sampling_loop_is_elitist_on_a_non_convex_cost():
    import torch
    from env_build_amd.mpc import first_minimum, sampling_loop
    from env_build_amd.sample import sample_tapes_reference, softmin_mean_reference
    H, B, S, iterations = 6, 12, 48, 8
    cost = bumpy_cost(H, B)
    calls = []

    def step(nominal, counter, sigma):
        calls.append((counter, sigma))
        U = sample_tapes_reference(nominal, S, 21, counter, sigma, beta=0.5)
        J = cost(U)
        mean, idx = softmin_mean_reference(U, J, 2.0)
        assert torch.equal(idx, first_minimum(J))
        best = U.gather(0, idx.view(1, 1, B, 1).expand(1, H, B, 2))[0]
        return J[0], best, J.gather(0, idx.view(1, B))[0], mean
    u0 = torch.full((H, B, 2), 1.5)                          # beyond the box: the loop clamps its start
    u, J, info = sampling_loop(step, u0, iterations, (0.5, 0.4), sigma_decay=0.5, counter=100)
    hist = info['J_history']
    assert hist.shape == (iterations + 1, B) and info['counter_next'] == 100 + iterations
    assert [c for c, _ in calls] == list(range(100, 100 + iterations))
    assert calls[0][1] == (0.5, 0.4) and calls[3][1] == (0.5 * 0.5 ** 3, 0.4 * 0.5 ** 3)
    ok = hist[:, :-1]
    assert bool(torch.isfinite(ok).all()) and bool((ok[1:] <= ok[:-1]).all())         # it never increases
    assert bool((ok[-1] < ok[0]).all())                                               # and every env improves on the start
    assert torch.equal(hist[-1, :-1], J[:-1])
    assert float(u.abs().max()) <= 1.0
    assert torch.equal(cost(u.unsqueeze(0))[0, :-1], J[:-1])                          # J is the cost of the returned tape
    # the NaN env keeps its start
    assert bool(torch.isnan(hist[:, -1]).all()) and torch.equal(u[:, -1], torch.ones((H, 2)))
    u2, J2, _ = sampling_loop(step, u0, iterations, (0.5, 0.4), sigma_decay=0.5, counter=100)
    assert torch.equal(u2, u) and torch.equal(J2[:-1], J[:-1])                        # the same counter: the same bits
