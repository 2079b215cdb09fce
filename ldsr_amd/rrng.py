"""R-compatible uniform random numbers: R's default generator is
Mersenne-Twister seeded by set.seed() through an LCG scrambler (R sources, src/main/RNG.c:
RNG_Init / MT_genrand / fixup).  With it `make_init(p, q, n, r_seed=k)` reproduces what
`set.seed(k); make_init(p, q, n)` draws in R (reference R/LDS_reconstruction.R:14-30), so a
reconstruction can be replayed without shipping the init list across the boundary.

Normal draws follow R's default inversion rule (RUniform.rnorm), so the uniforms LDS_rep would
consume after set.seed(k) can be handed to the GPU simulator (ldsr_amd/sim.py).

R is not available in this image; the implementation is pinned in tests by the widely
published first draws of set.seed(1), set.seed(42) and set.seed(123)."""
import numpy as np

_I2_32M1 = 2.328306437080797e-10      # 1/(2^32 - 1), R's fixup constant
_SCALE = 2.3283064365386963e-10       # 2^-32


class RUniform:
    def __init__(self, seed):
        s = np.uint32(int(seed) & 0xFFFFFFFF)
        with np.errstate(over="ignore"):
            for _ in range(50):                       # initial scrambling
                s = np.uint32(69069) * s + np.uint32(1)
            key = np.empty(625, dtype=np.uint32)
            for j in range(625):
                s = np.uint32(69069) * s + np.uint32(1)
                key[j] = s
        # FixupSeeds: dummy[0] = mti = 624 -> regenerate on first use; mt = dummy + 1
        self._bg = np.random.MT19937()
        self._bg.state = {"bit_generator": "MT19937", "state": {"key": key[1:], "pos": 624}}

    def unif_rand(self, n=1):
        x = self._bg.random_raw(n).astype(np.float64) * _SCALE
        x = np.where(x <= 0.0, 0.5 * _I2_32M1, x)
        x = np.where(1.0 - x <= 0.0, 1.0 - 0.5 * _I2_32M1, x)
        return x

    def runif(self, n, a=0.0, b=1.0):
        return a + (b - a) * self.unif_rand(n)

    def norm_rand(self, n=1):
        """n draws of R's norm_rand() with the default normal.kind = "Inversion" (nmath snorm.c):
        two uniforms per draw, u = (int)(2^27 u1) + u2, z = qnorm(u / 2^27)."""
        u = self.unif_rand(2 * int(n)).reshape(-1, 2)
        return qnorm((np.floor(_BIG * u[:, 0]) + u[:, 1]) / _BIG)

    def rnorm(self, n, mean=0.0, sd=1.0):
        """R's rnorm(n, mean, sd) for scalar mean and sd (nmath rnorm.c): a NaN mean or a NaN,
        negative or infinite sd gives NaN, sd = 0 or an infinite mean gives the mean, both without
        consuming a uniform; otherwise mean + sd * norm_rand()."""
        mean, sd = float(mean), float(sd)
        if np.isnan(mean) or not np.isfinite(sd) or sd < 0.0:
            return np.full(int(n), np.nan)
        if sd == 0.0 or not np.isfinite(mean):
            return np.full(int(n), mean)
        return mean + sd * self.norm_rand(n)


_BIG = 134217728.0                    # 2^27, R's BIG in norm_rand

# Wichura's AS 241 (PPND16) coefficients, highest power first, as R's nmath qnorm.c uses them
_A = (2509.0809287301226727, 33430.575583588128105, 67265.770927008700853, 45921.953931549871457,
      13731.693765509461125, 1971.5909503065514427, 133.14166789178437745, 3.387132872796366608)
_B = (5226.495278852545925, 28729.085735721942674, 39307.89580009271061, 21213.794301586595867,
      5394.1960214247511077, 687.1870074920579083, 42.313330701600911252, 1.0)
_C = (7.7454501427834140764e-4, .0227238449892691845833, .24178072517745061177, 1.27045825245236838258,
      3.64784832476320460504, 5.7694972214606914055, 4.6303378461565452959, 1.42343711074968357734)
_D = (1.05075007164441684324e-9, 5.475938084995344946e-4, .0151986665636164571966, .14810397642748007459,
      .68976733498510000455, 1.6763848301838038494, 2.05319162663775882187, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, .0012426609473880784386, .026532189526576123093,
      .29656057182850489123, 1.7848265399172913358, 5.4637849111641143699, 6.6579046435011037772)
_F = (2.04426310338993978564e-15, 1.4215117583164458887e-7, 1.8463183175100546818e-5, 7.868691311456132591e-4,
      .0148753612908506148525, .13692988092273580531, .59983220655588793769, 1.0)


def _horner(c, r):
    out = np.full_like(r, c[0])
    for k in c[1:]:
        out = out * r + k
    return out


def qnorm(p):
    """R's qnorm(p, 0, 1) (AS 241) elementwise for p in (0, 1).  R's extra steps for
    sqrt(-log(min(p, 1 - p))) > 27 (p below ~1e-316) are left out: the draws above have p >= 2^-81."""
    p = np.asarray(p, dtype=np.float64)
    q = p - 0.5
    out = np.empty_like(p)
    c = np.abs(q) <= 0.425
    r = 0.180625 - q[c] * q[c]
    out[c] = q[c] * _horner(_A, r) / _horner(_B, r)
    t = ~c
    r = np.sqrt(-np.log(np.where(q[t] > 0, 0.5 - p[t] + 0.5, p[t])))
    lo = r <= 5.0
    val = np.empty_like(r)
    val[lo] = _horner(_C, r[lo] - 1.6) / _horner(_D, r[lo] - 1.6)
    val[~lo] = _horner(_E, r[~lo] - 5.0) / _horner(_F, r[~lo] - 5.0)
    out[t] = np.where(q[t] < 0, -val, val)
    return out


def make_init_packed_r(p, q, n, r_seed):
    """Packed [n, 6+p+q] thetas drawn exactly as R's make_init after set.seed(r_seed):
    per restart runif(1), runif(p,-1,1), runif(1), runif(q,-1,1)."""
    g = RUniform(r_seed)
    th = np.empty((n, 6 + p + q))
    for r in range(n):
        th[r, 0] = g.runif(1)[0]
        th[r, 1:1 + p] = g.runif(p, -1.0, 1.0)
        th[r, 1 + p] = g.runif(1)[0]
        th[r, 2 + p:2 + p + q] = g.runif(q, -1.0, 1.0)
    th[:, 2 + p + q] = 1.0
    th[:, 3 + p + q] = 1.0
    th[:, 4 + p + q] = 0.0
    th[:, 5 + p + q] = 1.0
    return th
