"""Helper of the radiance tests: reflect_ray, refract_ray, the bounce loop of secondary_light and the two colour rules of
draw_pixel (oracle/rt_oracle.c:189-266, kernels.cl:54-88, :342-365, :416-423) restated in numpy FP32.  Closest hits and shadow
masks come from callables — the oracle's closest_hit / in_shadow or the product's brute-force diagnostic — and the direct
light is shade_util.direct_light itself, so that the same restatement is the yardstick on the CPU
(tests/test_radiance_util_cpu.py pins it to Oracle.render on every pixel) and on the GPU (tests/test_gpu_radiance.py)."""
import numpy as np

import shade_util as su

F = np.float32
AIR, GLASS = F(1.0), F(1.52)


def dot(a, b):
    """x*x + y*y + z*z, left to right"""
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F) + a[:, 2] * b[:, 2]).astype(F)


def normalize(v):
    """v / sqrtf(x*x + y*y + z*z)"""
    return (v / np.sqrt(dot(v, v)).astype(F)[:, None]).astype(F)


def reflect_ray(direction, point, normal):
    """-> (start, direction, medium) of the reflected ray, rt_oracle.c:189-198"""
    dn = dot(direction, normal)
    d = (direction - F(2.0) * (dn[:, None] * normal).astype(F)).astype(F)
    start = (point + F(0.0001) * d).astype(F)
    return start, normalize(d), np.full(len(d), AIR, F)


def refract_ray(direction, point, normal, medium):
    """-> (start, direction, medium) of the refracted ray, rt_oracle.c:201-219"""
    air = medium == AIR
    n1 = np.where(air, AIR, GLASS).astype(F)
    n2 = np.where(air, GLASS, AIR).astype(F)
    c1 = dot(normal, direction)
    normal = np.where((c1 < 0)[:, None], (F(-1.0) * normal).astype(F), normal).astype(F)
    c1 = np.abs(c1)
    n = (n1 / n2).astype(F)
    c2 = np.sqrt(F(1.0) - ((n * n).astype(F) * (F(1.0) - (c1 * c1).astype(F)).astype(F)).astype(F)).astype(F)
    d = ((n[:, None] * direction).astype(F) + (((n * c1).astype(F) - c2).astype(F)[:, None] * (-normal)).astype(F)).astype(F)
    start = (point + F(0.0001) * d).astype(F)
    out = [start, normalize(d), n2]
    tir = c2 < 0                                                 # (unreachable: the sqrt of a negative is NaN)
    if tir.any():
        r = reflect_ray(direction[tir], point[tir], normal[tir])
        for o, v in zip(out, r):
            o[tir] = v
    return tuple(out)


def in_domain(rays):
    """The domain of the exact culls (include/uob_rt.h): finite, every |coordinate| <= 2^16, max |direction component| >= 2^-20;
    a ray outside it (a NaN bounce ray behind a total internal reflection included) is traced without culling"""
    with np.errstate(all="ignore"):
        r = np.asarray(rays, F).reshape(-1, 6)
        return (np.abs(r) <= F(65536.0)).all(1) & (np.abs(r[:, 3:6]).max(1) >= F(2.0 ** -20))


def radiance(rays, seeds, light, samples, spread, max_bounces, closest_hit, in_shadow):
    """One AA sample's colour for every ray [k,6] = (start, direction as given), seeds int32 [k] (None: k & 0xFFFFFF).
    closest_hit(rays [m,6]) -> (tri [m], out10 [m,10]); in_shadow(rays [m,6], radius_sq [m]) -> 0/1 [m].
    Returns dict: rgba float32 [k,4] (w = the first hit exists), prim int32 [k] (the first hit), bounces int32 [k] (bounce
    rays traced for the ray), diffuse bool [k] (a diffuse surface was reached), specular bool [k] (the first hit is mirror
    or glass), unculled int (rays of any kind — caller, bounce, sample — outside in_domain; the sample rays of a point whose
    term is 0 are not traced and do not count)."""
    with np.errstate(all="ignore"):
        rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
        k = len(rays)
        seeds = (np.arange(k) & 0xFFFFFF).astype(np.int32) if seeds is None else np.asarray(seeds, np.int32).reshape(-1)
        tri, o10 = closest_hit(rays)
        tri, o10 = np.asarray(tri).reshape(-1), np.asarray(o10, F).reshape(-1, 10)
        unculled = int((~in_domain(rays)).sum())
        prim = tri.astype(np.int32).copy()
        hit = tri != -1
        P, N, col = o10[:, 0:3].copy(), o10[:, 3:6].copy(), o10[:, 6:10].copy()
        direction = rays[:, 3:6].copy()
        medium = np.full(k, AIR, F)
        specular = hit & (col[:, 3] <= 0)                       # :260
        diffuse = hit & ~specular
        bounced = np.zeros(k, bool)
        go = specular.copy()
        bounces = np.zeros(k, np.int32)
        for _ in range(max_bounces):                            # :224, all rays still on a specular surface at once
            idx = np.flatnonzero(go)
            if idx.size == 0:
                break
            bounces[idx] += 1
            mirror = col[idx, 3] == 0
            s, d, m = refract_ray(direction[idx], P[idx], N[idx], medium[idx])
            if mirror.any():
                rs, rd, rm = reflect_ray(direction[idx][mirror], P[idx][mirror], N[idx][mirror])
                s[mirror], d[mirror], m[mirror] = rs, rd, rm
            bounce = np.ascontiguousarray(np.concatenate([s, d], 1), F)
            unculled += int((~in_domain(bounce)).sum())
            t, o = closest_hit(bounce)
            t, o = np.asarray(t).reshape(-1), np.asarray(o, F).reshape(-1, 10)
            h = t != -1
            P[idx], N[idx], col[idx] = o[:, 0:3], o[:, 3:6], o[:, 6:10]
            direction[idx], medium[idx] = d, m
            lit = h & (o[:, 9] > 0)                             # :228
            diffuse[idx[lit]] = True
            bounced[idx[lit]] = True
            go[idx] = h & (o[:, 9] <= 0)                        # (a miss leaves the bounce ray's own w = 1: the loop ends)
        rgba = np.zeros((k, 4), F)
        rgba[:, 3] = hit.astype(F)
        if diffuse.any():
            L, _, term = su.direct_light(P[diffuse], N[diffuse], seeds[diffuse], light, samples, spread, in_shadow)
            srays, _ = su.sample_rays(P[diffuse], N[diffuse], seeds[diffuse], light, samples, spread)
            unculled += int((~in_domain(srays[~(term == 0)])).sum())
            l = (F(0.5) + L).astype(F)
            first = (col[diffuse][:, :3] * l[:, None]).astype(F)                          # :263-264
            behind = ((F(0.9) * l).astype(F)[:, None] * col[diffuse][:, :3]).astype(F)    # :229-230
            rgba[diffuse, :3] = np.where(bounced[diffuse][:, None], behind, first)
        return {"rgba": rgba, "prim": prim, "bounces": bounces, "diffuse": diffuse, "specular": specular,
                "unculled": unculled}


def pixel_colour(rgb_samples):
    """[..., aa, 3] -> [..., 3]: the float32 sum in sample order, then / aa (draw_pixel, rt_oracle.c:261-270)"""
    aa = rgb_samples.shape[-2]
    acc = np.zeros(rgb_samples.shape[:-2] + (3,), F)
    for a in range(aa):
        acc = (acc + rgb_samples[..., a, :]).astype(F)
    return (acc / F(aa)).astype(F)
