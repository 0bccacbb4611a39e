"""Models with first-order linear recurrences (symbolic.linear_recurrence / cumsum) for the CPU and GPU scan tests."""
import numpy as np

from nutpie_amd import symbolic as S


def scan_model(R: int, T: int, a_kind: str = "scalar", init_kind: str = "param", seed: int = 0, deterministic: bool = False, latent: bool = True):
    """z ~ N(0, 1) on R rows of T steps, x = linear_recurrence(a, s z, init) along the steps, y ~ N(x, 1) with data y.
    latent=False: z is data instead of a parameter (a long series with a handful of parameters).
    a_kind: "one" (a cumulative sum), "scalar" (a parameter in (-1, 1)), "vector" (tanh of a parameter per element);
    init_kind: "const", "param" (one scalar) or "row" (a parameter per row; R > 1)."""
    m = S.Model()
    if R > 1:
        m.dim("row", R)
        m.dim("time", T)
        dn, along = m.product("row", "time").name, "time"
    else:
        m.dim("time", T)
        dn, along = "time", None
    rng = np.random.default_rng(seed)
    z = m.param("z", dim=dn) if latent else m.data("w", rng.normal(size=R * T), dim=dn)
    s = m.param("s", lower=0.0)
    if a_kind == "one":
        a = 1.0
    elif a_kind == "scalar":
        a = m.param("phi", lower=-1.0, upper=1.0)
    else:
        a = S.tanh(m.param("av", dim=dn))
    if init_kind == "const":
        init = 0.25
    elif init_kind == "param":
        init = m.param("x0")
        m.add_logp(S.normal_lpdf(init, 0.0, 1.0))
    else:
        init = m.param("x0r", dim="row")
        m.add_logp(S.normal_lpdf(init, 0.0, 1.0).sum())
    y = m.data("y", 0.5 * rng.normal(size=R * T), dim=dn)
    m.add_logp((S.normal_lpdf(z, 0.0, 1.0).sum() if latent else 0.0) + S.halfnormal_lpdf(s, 1.0))
    x = S.linear_recurrence(a, s * z, init=init, along=along)
    m.add_logp(S.normal_lpdf(y, x, 1.0).sum())
    if deterministic:
        m.deterministic("path", x)
    return m


def points(n_dim: int, n: int, seed: int, scale: float = 0.3) -> np.ndarray:
    return scale * np.random.default_rng(seed).normal(size=(n, n_dim))
