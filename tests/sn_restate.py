"""Plain-torch restatement of spectral normalisation as torch.nn.utils.spectral_norm does it in its hook form with default arguments
(one power iteration, eps 1e-12, dim 0) -- the arithmetic csrc/spectral_norm.hip implements -- in whatever dtype it is given (fp64
for the references, fp32 for the yardsticks).  A weight is the matrix [rows = Cout][K = Cin kh kw] in OIHW row order.

Shared by tools/make_golden_spectral_norm.py (which asserts it equal to the reference's modules), tests/test_cpu_spectral_norm.py and
tests/test_gpu_spectral_norm.py.  Inputs are pure functions of seeds."""
import torch

EPS = 1e-12

# the kernel-level job table of the GPU test: a one-row matrix (u = +-1), rows that are no multiple of 4 or 64, more row blocks than one
# workgroup takes, a row longer than one block's pass, and the largest matrix of the shipped discriminators
MATRICES = [(1, 128), (5, 27), (64, 48), (8, 100), (128, 1024), (3, 4100), (512, 4096)]
ITERATIONS = 3

# the network-level cases: constructor arguments and input shape
NETS = {"patchgan": (dict(input_nc=3, ndf=8, n_layers=3, use_spectral_norm=True), (2, 3, 32, 32)),
        "unet": (dict(input_nc=3, nf=16, spectral_norm=True), (2, 3, 16, 16))}
NET_SEED = 4242


def normalize(x, eps=EPS):
    return x / torch.clamp(x.norm(), min=eps)


def iterate(W, u, v, eps=EPS):
    """One power iteration over the [rows, K] matrix W -> (u', v')."""
    v = normalize(W.t().mv(u), eps)
    u = normalize(W.mv(v), eps)
    return u, v


def sigma(W, u, v):
    return torch.dot(u, W.mv(v))


def forward(W, u, v, training=True, eps=EPS):
    """-> (W / sigma, u', v', sigma) of one forward; in eval mode u and v come back unchanged."""
    if training:
        u, v = iterate(W, u, v, eps)
    s = sigma(W, u, v)
    return W / s, u, v, s


def grad_correction(G, Wn, u, v, s):
    """dL/dW from G = dL/d(W / sigma), with u and v constants: (G - <G, W / sigma> u v^T) / sigma."""
    return (G - (G * Wn).sum() * torch.outer(u, v)) / s


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def matrix_case(i):
    """fp64 (W, u0, v0, G) of MATRICES[i]; u0 and v0 are unit vectors as the reference's buffers are."""
    rows, K = MATRICES[i]
    W = rnd(rows, K, seed=9100 + i, scale=0.1)
    u0, v0 = normalize(rnd(rows, seed=9200 + i)), normalize(rnd(K, seed=9300 + i))
    return W, u0, v0, rnd(rows, K, seed=9400 + i)


def matrix_run(i, dtype):
    """ITERATIONS consecutive training forwards over matrix_case(i), then the correction of the planted G against the last of them
    -> dict u, v, sigma, wn, grad (in `dtype`; inputs rounded to it first)."""
    W, u, v, G = (t.to(dtype) for t in matrix_case(i))
    for _ in range(ITERATIONS):
        Wn, u, v, s = forward(W, u, v)
    return dict(u=u, v=v, sigma=s.reshape(1), wn=Wn, grad=grad_correction(G, Wn, u, v, s))


def perturb_(net):
    """The in-place weight change in front of the recorded eval forward: every parameter, by name, plus a seeded field of +-0.02."""
    with torch.no_grad():
        for i, (k, p) in enumerate(sorted(net.named_parameters())):
            p.add_(rnd(*p.shape, seed=600 + i, scale=0.02).to(device=p.device, dtype=p.dtype))


def net_inputs(name):
    """fp64 (x1, x2, g1, g2): two different inputs and the two output gradients of the recorded sequence (g shapes are the outputs')."""
    shape = NETS[name][1]
    oshape = (shape[0], 1, shape[2], shape[3]) if name == "unet" else (shape[0], 1, shape[2] // 8 - 2, shape[3] // 8 - 2)
    return rnd(*shape, seed=51), rnd(*shape, seed=52), rnd(*oshape, seed=53), rnd(*oshape, seed=54)
