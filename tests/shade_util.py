"""Helper of the shade tests: direct_light (oracle/rt_oracle.c:168-186, kernels.cl:313-340) restated in numpy FP32, with the
shadow masks taken from a callable — the oracle's in_shadow or the product's ray queries — so that the same restatement is the
yardstick on the CPU (tests/test_shade_util_cpu.py pins it to Oracle.render) and on the GPU (tests/test_gpu_shade.py)."""
import numpy as np

F = np.float32
U = np.uint32


def xorshift(s):
    s = s ^ (s << U(13))
    s = s ^ (s >> U(17))
    return s ^ (s << U(5))


def jitter_states(seeds, samples):
    """uint32 [k, samples, 3]: the generator's state for every sample (one step after the seeds, then one per sample)."""
    g = np.asarray(seeds, np.int32).reshape(-1)
    gf = g.astype(F)
    r = np.stack([g.astype(U), (gf * F(91.0)).astype(np.int64).astype(U), (gf * F(19.0)).astype(np.int64).astype(U)], 1)
    r = xorshift(r)
    out = np.zeros((len(g), samples, 3), U)
    for i in range(samples):
        r = xorshift(r)
        out[:, i] = r
    return out


def crush(r, spread):
    spread = F(spread)
    return ((spread * r.astype(F)).astype(F) / F(4294967296.0)).astype(F) - spread / F(2.0)


def setup(points, normals, light):
    """dir, start, radius_sq and the numerator / denominator of the per-sample term, all float32"""
    p = np.asarray(points, F).reshape(-1, 3)
    n = np.asarray(normals, F).reshape(-1, 3)
    d = (np.asarray(light, F)[:3] - p).astype(F)
    start = (p + F(0.0001) * d).astype(F)
    rsq = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)
    dot = ((d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]).astype(F) + d[:, 2] * n[:, 2]).astype(F)
    num = (F(16.0) * np.fmax(dot, F(0.0))).astype(F)            # C's fmaxf: the number when one operand is NaN
    den = (F(4.0) * F(3.14159274) * rsq).astype(F)
    return d, start, rsq, num, den


def sample_rays(points, normals, seeds, light, samples, spread):
    """rays float32 [k, samples, 6] and radius_sq [k, samples] of direct_light's shadow tests"""
    d, start, rsq, _, _ = setup(points, normals, light)
    jit = crush(jitter_states(seeds, samples), spread)
    sd = (d[:, None, :] + jit).astype(F)
    rays = np.concatenate([np.broadcast_to(start[:, None, :], sd.shape), sd], 2)
    return np.ascontiguousarray(rays, F), np.ascontiguousarray(np.broadcast_to(rsq[:, None], sd.shape[:2]), F)


def direct_light(points, normals, seeds, light, samples, spread, in_shadow):
    """(light float32 [k], unshadowed int32 [k], term float32 [k]); in_shadow(rays [m,6], radius_sq [m]) -> 0/1 [m]"""
    with np.errstate(all="ignore"):
        _, _, _, num, den = setup(points, normals, light)
        rays, r2 = sample_rays(points, normals, seeds, light, samples, spread)
        k = rays.shape[0]
        blocked = np.asarray(in_shadow(rays.reshape(-1, 6), r2.reshape(-1))).reshape(k, samples) != 0
        mask = (~blocked).astype(F)
        total = np.zeros(k, F)
        for i in range(samples):
            total = (total + ((mask[:, i] * num).astype(F) / den).astype(F)).astype(F)
        return (total / F(samples)).astype(F), (~blocked).sum(1).astype(np.int32), (num / den).astype(F)


def u32(a):
    return np.ascontiguousarray(a, F).view(U)


def same_bits(got, want):
    """Equal bit for bit; two NaNs count as equal when both are quiet or both signalling (their class): a NaN's sign and
    payload are whatever the machine's 0/0 or inf - inf produces and differ between an x86 host and the GPU."""
    g, w = u32(got), u32(want)
    nan = np.isnan(got) & np.isnan(want) & (((g >> U(22)) & U(1)) == ((w >> U(22)) & U(1)))
    return (g == w) | nan


def pixel_ids(rows, width):
    return (np.asarray(rows, np.int64)[:, None] * width + np.arange(width)[None, :]).astype(np.int32)
