"""Float64 definitions of the kernels of csrc/bn_train.hip (training-mode BatchNorm2d statistics with the running update, the
fused normalise / activation forward, the two backward sums and the input gradient; the softmax cross-entropy): plain torch on
the CPU, written from the formulas of nn.BatchNorm2d / nn.CrossEntropyLoss.  No HIP, none of the project's ops.  Tensors are
[B, C, H, W]; every input is promoted to float64.

As in tests/_ew_defs.py a result that is a sum comes as Sum(value, abs_terms): abs_terms is the same formula applied to the
absolute values of its terms.  A kernel output is held to  |got - value| <= c * 2^-24 * abs_terms  with the constant c of
that kernel, DERIVED HERE from the kernel's reduction shape (u = 2^-24, the unit roundoff of fp32):

  Reduced quantities (mean, var, running statistics, dbeta, dgamma, the mean loss).  Every first-stage block, every tree
  level and the combine of the chunk partials accumulate in fp64: a lane adds its elements (at most chunk / 256 = 32 per
  16-byte lane component, any number when the chunk grows) in fp64, then 6 shuffle levels, 2 levels over the waves, 8 + 2
  levels over the <= 256 chunk partials.  An fp64 sum of n terms t_i in any order is within n * 2^-53 * sum |t_i| of the
  exact one; each term (x, (x - mean)^2, g * xhat) is itself formed in fp64 from fp32 inputs with at most 4 fp64 roundings.
  With n < 2^31 the whole fp64 part stays below 2^-20 u * abs_terms.  What remains is the ONE rounding of the result to fp32:
  u * |value| <= u * abs_terms.  So the reduction error is (1 + 2^-20) u abs_terms, and

    C_MEAN = C_VAR = C_DBETA = C_DGAMMA = 2   (1 for the final rounding, 1 spare for: the fp64 part; in var, the division by n
                                               and the mean being a rounded fp64 value — (mean_hat - mean)^2 is second order;
                                               in dgamma, invstd: the sum var + eps is an fp32 add (ATen's arithmetic), a
                                               relative u / 2 on invstd and so on every term, then an fp64 sqrt and division)
    C_RUNNING = 2                             (1 - m) rm + m stat evaluated in fp64 from the fp64 statistic, rounded once

  Element-wise outputs, fp32 arithmetic per element with per-channel constants formed in fp64 and rounded once:
    forward   d = x - mean (1 rounding on the |x - mean| s term), s = fl(gamma * invstd) (1), fma(d, s, beta) (1 on the
              whole pre-activation), + residual (1 on the whole): 4 on the first term, 2 on beta, 1 on the residual;
              the fp32 add var + eps inside invstd (1/2 on the first term), second-order terms: C_FWD = 5.  ReLU / ReLU6 are
              1-Lipschitz and exact.
    apply     gx = fma(-(d * inv), k2, g - k1) * s with d = x - mean (1), inv = fl(invstd) (1), d * inv (1), k2 = fl(dgamma / n)
              (1), k1 = fl(dbeta / n) (1), g - k1 (1), the fma (1), s = fl(gamma invstd) (1), the product (1): the xhat k2
              term passes 7 roundings, k1 5, g 4; the fp32 add var + eps adds 1/2 through inv and 1/2 through s: 8 on
              the largest term, second-order terms: C_APPLY = 8.5.
  dgamma / n and dbeta / n take the kernel's own fp32 dgamma, dbeta (inputs of the apply launch), the gate the kernel's own y.

  Cross-entropy: the bound is the sibling loss kernels' (tests/test_hip_parity.py, test_fused_loss_kernels_match_the_torch_
  compositions): max error <= 2e-6 * max(1e-3, max |reference|).

tests/test_bn_train_defs_cpu.py ties these to F.batch_norm / F.cross_entropy and autograd and shows that the bounds have
teeth; tests/test_bn_train_gpu.py holds the kernels to them."""
import collections

import torch
import torch.nn.functional as F

F64 = torch.float64
U = 2.0 ** -24
Sum = collections.namedtuple("Sum", "value abs_terms")

C_MEAN = C_VAR = C_DBETA = C_DGAMMA = C_RUNNING = 2.0
C_FWD = 5.0
C_APPLY = 8.5
CE_TOL = 2e-6

ACTS = ("none", "relu", "relu6")
SHAPES = ((2, 1, 1), (1, 3, 49), (3, 24, 49), (4, 160, 49), (2, 16, 196), (5, 7, 3136), (8, 4, 12544))  # (B, C, HW)
HW2 = {1: (1, 1), 49: (7, 7), 196: (14, 14), 3136: (56, 56), 12544: (112, 112)}


def gen_inputs(shape, kind, seed=0):
    """The GPU test's own inputs, fp32: x ('gauss': N(1, 1); 'shifted': 100 + 0.01 N(0, 1)), gy, residual ~ N(0, 1),
    gamma ~ N(1, 0.3), beta ~ N(0, 0.5), running statistics."""
    b, c, hw = shape
    h, w = HW2[hw]
    g = torch.Generator().manual_seed(1000 * seed + 17 * b + 3 * c + hw)
    z = torch.randn(b, c, h, w, generator=g)
    x = (1.0 + z) if kind == "gauss" else (100.0 + 0.01 * z)
    return dict(x=x.float(), gy=torch.randn(b, c, h, w, generator=g), res=torch.randn(b, c, h, w, generator=g),
                gamma=1.0 + 0.3 * torch.randn(c, generator=g), beta=0.5 * torch.randn(c, generator=g),
                rm=torch.randn(c, generator=g), rv=torch.rand(c, generator=g) + 0.5)


def _chan(v):
    return v.to(F64).view(1, -1, 1, 1)


def count(x):
    return x.shape[0] * x.shape[2] * x.shape[3]


def mean(x):
    x = x.to(F64)
    n = count(x)
    return Sum(x.sum(dim=(0, 2, 3)) / n, x.abs().sum(dim=(0, 2, 3)) / n)


def var(x):
    """Biased variance: the mean of (x - mean)^2; all terms are >= 0, abs_terms is the value."""
    x = x.to(F64)
    v = ((x - _chan(mean(x).value)) ** 2).sum(dim=(0, 2, 3)) / count(x)
    return Sum(v, v.clone())


def running(stat, old, momentum, unbias=1.0):
    """(1 - m) old + m stat * unbias (unbias = n / (n - 1) for the variance)."""
    old, m = old.to(F64), float(momentum)
    return Sum((1 - m) * old + m * stat.value * unbias, (1 - m) * old.abs() + m * stat.abs_terms * unbias)


def invstd(v, eps):
    return 1.0 / torch.sqrt(v.to(F64) + float(eps))


def activate(v, act):
    if act == "relu":
        return v.clamp(min=0.0)
    if act == "relu6":
        return v.clamp(min=0.0, max=6.0)
    assert act == "none", act
    return v


def gate(y, act):
    """The backward's gate from the SAVED output y: relu y > 0, relu6 0 < y < 6, none: open."""
    y = y.to(F64)
    if act == "relu":
        return (y > 0).to(F64)
    if act == "relu6":
        return ((y > 0) & (y < 6)).to(F64)
    return torch.ones_like(y)


def bn_act_fwd(x, mu, v, gamma, beta, eps, res=None, act="none"):
    """act((x - mu) * invstd * gamma + beta (+ res)); abs_terms of the pre-activation."""
    x = x.to(F64)
    t = (x - _chan(mu)) * _chan(invstd(v, eps) * gamma.to(F64))
    pre, a = t + _chan(beta), t.abs() + _chan(beta).abs()
    if res is not None:
        pre, a = pre + res.to(F64), a + res.to(F64).abs()
    return Sum(activate(pre, act), a)


def xhat(x, mu, v, eps):
    return (x.to(F64) - _chan(mu)) * _chan(invstd(v, eps))


def bwd_sums(gy, y, x, mu, v, eps, act="none", keep=None):
    """(dbeta, dgamma) = (sum g, sum g * xhat), g = gy * gate(y).  keep: an optional 0/1 mask of the elements that take part
    (the teeth test drops one)."""
    g = gy.to(F64) * gate(y, act) if act != "none" else gy.to(F64)
    if keep is not None:
        g = g * keep
    t = g * xhat(x, mu, v, eps)
    return Sum(g.sum(dim=(0, 2, 3)), g.abs().sum(dim=(0, 2, 3))), Sum(t.sum(dim=(0, 2, 3)), t.abs().sum(dim=(0, 2, 3)))


def bwd_apply(gy, y, x, mu, v, gamma, dgamma, dbeta, eps, act="none"):
    """gx = gamma * invstd * (g - dbeta / n - xhat * dgamma / n) and gres = g."""
    n = count(x)
    g = gy.to(F64) * gate(y, act) if act != "none" else gy.to(F64)
    s = _chan(gamma.to(F64) * invstd(v, eps))
    xh = xhat(x, mu, v, eps)
    k1, k2 = _chan(dbeta) / n, _chan(dgamma) / n
    return Sum(s * (g - k1 - xh * k2), s.abs() * (g.abs() + k1.abs() + (xh * k2).abs())), g


def cross_entropy(logits, targets):
    """(mean of logsumexp - logit[target], per-row argmax with the lowest index on ties)."""
    z = logits.to(F64)
    lse = torch.logsumexp(z, dim=1)
    loss = (lse - z.gather(1, targets.view(-1, 1)).squeeze(1)).mean()
    first_max = (z == z.max(dim=1, keepdim=True).values).to(torch.int8).argmax(dim=1)
    return loss, first_max


def cross_entropy_grad(logits, targets, g=1.0):
    z = logits.to(F64)
    p = torch.softmax(z, dim=1)
    return (p - F.one_hot(targets, z.shape[1]).to(F64)) * float(g) / z.shape[0]


def ce_inputs(b, k, seed=0):
    """Logits with +-80 entries and exact ties (also for the maximum), targets in range."""
    g = torch.Generator().manual_seed(77 + 1000 * seed + 13 * b + k)
    z = torch.randn(b, k, generator=g) * 3
    z[0, 0] = 80.0
    z[b // 2, k - 1] = -80.0
    if b > 1:
        z[1, :] = z[1, 0]  # a whole row of ties: argmax 0
    if b > 2 and k > 2:
        z[2, k - 1] = z[2, 1] = z[2].max() + 1  # a tied maximum: the lower index wins
    t = torch.randint(0, k, (b,), generator=g)
    t[0] = 0
    return z.float(), t
