"""CPU restatement of the Lion update, test infrastructure beside eval_ref.py / prep_ref.py: the four lines
of the update rule in NumPy float64, with the hyper-parameters rounded first as the kernel sees them, the error bounds that
follow from "at most four fp32 roundings per output", and the set of elements whose update direction fp32 rounding may decide.

    g' = g / grad_scale
    p <- p * (1 - lr * wd);   u = sign(beta1 * m + (1 - beta1) * g')  (sign(0) = 0);   p <- p - lr * u
    m <- beta2 * m + (1 - beta2) * g'
"""
import numpy as np

F = np.float32
EPS = 4.0 * 2.0 ** -24            # four roundings to nearest of a 24-bit significand


def hyper(lr, betas, weight_decay):
    """(lr, beta1, 1 - beta1, beta2, 1 - beta2, wd) as float64 values of what the kernel holds in fp32: float32(lr), float32(beta),
    float32(1) - float32(beta) (rounded to fp32), float32(wd)."""
    b1, b2 = F(betas[0]), F(betas[1])
    return tuple(float(v) for v in (F(lr), b1, F(F(1) - b1), b2, F(F(1) - b2), F(weight_decay)))


def lion_step(p, g, m, lr, betas, weight_decay, grad_scale=None):
    """One update in float64 from the fp32 state (p, m) and gradient g.  Returns a dict:
    p, m: the new values (float64);  p_tol, m_tol: the per-element error bounds of an fp32 evaluation;
    ambiguous: elements whose combination c = beta1 m + (1 - beta1) g' is within rounding of zero (their sign is not pinned)."""
    lr_, b1, omb1, b2, omb2, wd = hyper(lr, betas, weight_decay)
    p0, m0 = np.asarray(p, dtype=F).astype(np.float64), np.asarray(m, dtype=F).astype(np.float64)
    gp = np.asarray(g, dtype=F).astype(np.float64)
    if grad_scale is not None:
        gp = gp / float(F(grad_scale))
    c = b1 * m0 + omb1 * gp
    p1 = p0 * (1.0 - lr_ * wd) - lr_ * np.sign(c)
    m1 = b2 * m0 + omb2 * gp
    return {"p": p1, "m": m1,
            "p_tol": EPS * (np.abs(p0) + lr_),
            "m_tol": EPS * (np.abs(b2 * m0) + np.abs(omb2 * gp)),
            "ambiguous": np.abs(c) <= EPS * (np.abs(b1 * m0) + np.abs(omb1 * gp))}


AMBIGUOUS_CAP = 1e-5              # share of a test's elements that may be left out of the comparison of p


def check(p_new, m_new, ref, what=""):
    """Assert an fp32 result (p_new, m_new) against ``lion_step``'s dict: m everywhere, p outside the ambiguous set.  Prints the
    worst ratio error / bound of both before asserting."""
    pn, mn = np.asarray(p_new, dtype=np.float64), np.asarray(m_new, dtype=np.float64)
    keep = ~ref["ambiguous"]
    em = np.abs(mn - ref["m"])
    ep = np.abs(pn - ref["p"])
    # an exact zero bound (p = 0 cannot happen with lr > 0; m0 = g = 0 can): the result must then be exact
    rm = float(np.max(np.where(ref["m_tol"] > 0, em / np.where(ref["m_tol"] > 0, ref["m_tol"], 1.0), np.where(em > 0, np.inf, 0.0)), initial=0.0))
    rp = float(np.max((ep / ref["p_tol"])[keep], initial=0.0))
    print(f"{what}: worst |m - m_ref| / bound = {rm:.3f}, worst |p - p_ref| / bound = {rp:.3f}, ambiguous {int((~keep).sum())} of {keep.size}")
    assert rm <= 1.0, f"{what}: exp_avg off by {rm:.3f} x the four-rounding bound"
    assert rp <= 1.0, f"{what}: parameter off by {rp:.3f} x the four-rounding bound"
