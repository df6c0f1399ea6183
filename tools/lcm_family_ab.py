#!/usr/bin/env python3
"""Every output bit of the twelve latent-prep / LCM-step entries (csrc/lcm.hip) as SHA-256 digests, through whichever library FIE_LIB_PATH
names (fie_amd/hip.py): the A/B of a change that must not move a bit.  One process per library, one after the other:

    FIE_LIB_PATH=<parent build>/libfie_hip.so python tools/lcm_family_ab.py --out A.json
    python tools/lcm_family_ab.py --out B.json
    python tools/lcm_family_ab.py --compare A.json B.json        # exit status 1 and the differing cases, if any

tests/golden/lcm_family_digests.json is such a file, written on the library of the commit BEFORE the kernels were folded into one body each,
and tests/test_lcm_family_gpu.py runs cases() against it.  A case is a tuple whose str() is its key in the file; its inputs come from the seeded
CPU generators of tests/pointwise_check.py; its digest covers every output buffer whole, padding columns included, over a NaN prefill."""
import argparse
import functools
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HW_SMALL = (1, 257)                     # one thread; a partial second block
HW_BIG = 2048 * 256 + 3                 # the second trip of the grid-stride loop (2048 blocks of 256)
DTYPES = ("f16", "f32")                 # the context's storage type: the plain entries and their _f32 twins
MASKS = ("zeros", "ones", "random")
LEVEL_STEPS = ((1, 0), (2, 0), (2, 1), (4, 1), (255, 0), (255, 254))
FLAVOURS = [("plain",)] + [("masked", m) for m in MASKS] + [("levels",) + ks for ks in LEVEL_STEPS]
SOME_FLAVOURS = [("plain",), ("masked", "random"), ("levels", 4, 1)]
OUTPUTS = ((True, True, 1), (True, True, 2), (False, True, 1), (True, False, 2))       # (model_in, decode_in, copies)
SCALARS = ("t999", "t19", "synthetic")  # pointwise_check.lcm_scalar_sets()
PREPS = [("plain",), ("src",)] + [("content", m) for m in range(4)]


def cases():
    """The one case list.  ("lcm", dtype, flavour, hw, nb, ld_eps, last, outputs, scalars) and ("prep", dtype, entry, hw, copies)."""
    out = []
    for dt in DTYPES:
        # the arithmetic: every flavour, scalar set, nb and step kind at both small sizes
        out += [("lcm", dt, fl, hw, nb, 8, last, OUTPUTS[nb - 1], sc)
                for fl, hw, nb, last, sc in itertools.product(FLAVOURS, HW_SMALL, (1, 2), (False, True), SCALARS)]
        # the addressing: row strides and the optional outputs
        out += [("lcm", dt, fl, 257, nb, ld, last, o, "synthetic")
                for fl, nb, ld, last, o in itertools.product(SOME_FLAVOURS, (1, 2), (4, 8), (False, True), OUTPUTS)]
        # the loop's second trip: one scalar set only
        out += [("lcm", dt, fl, HW_BIG, 2, 8, False, OUTPUTS[1], "synthetic") for fl in SOME_FLAVOURS]
        out += [("lcm", dt, ("plain",), HW_BIG, 1, 4, True, OUTPUTS[0], "synthetic")]
        out += [("prep", dt, e, hw, copies) for e, hw, copies in itertools.product(PREPS, HW_SMALL, (1, 2))]
        out += [("prep", dt, e, HW_BIG, 2) for e in (("plain",), ("src",), ("content", 2), ("content", 3))]
    return list(dict.fromkeys(out))         # the two grids overlap in a few cases


@functools.lru_cache(maxsize=4)
def _lcm_inputs(dt, hw, nb, ld_eps):
    """(pointwise_check.lcm_case without scalars, z0 f32 [hw, 4], n_init f32 [4, hw], {mask name: u8 [hw]}, levels u8 [hw]) on the CPU."""
    import torch
    import pointwise_check as pc
    case = pc.lcm_case(hw, ld_eps, nb, True, None, 1000 + hw % 1000 + 10 * nb + ld_eps, "cpu", torch.float16 if dt == "f16" else torch.float32)
    g = pc._gen(77 + hw % 1000)
    z0, n_init = pc._randn((hw, 4), g, "cpu"), pc._randn((4, hw), g, "cpu")
    masks = {"zeros": torch.zeros(hw, dtype=torch.uint8), "ones": torch.ones(hw, dtype=torch.uint8),
             "random": torch.randint(0, 2, (hw,), generator=g, dtype=torch.uint8)}
    return case, z0, n_init, masks, torch.randint(0, 256, (hw,), generator=g, dtype=torch.uint8)


@functools.lru_cache(maxsize=4)
def _prep_inputs(dt, hw):
    import torch
    import pointwise_check as pc
    case = pc.prep_case(hw, 2000 + hw % 1000, "cpu", torch.float16 if dt == "f16" else torch.float32)
    return case, torch.randint(0, 2, (hw,), generator=pc._gen(88 + hw % 1000), dtype=torch.uint8)


def _digest(named):
    import torch
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for name, t in named:
        if t is not None:
            h.update(name.encode())
            h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_case(case):
    """The case's digest, on the library this process loaded."""
    import torch
    import pointwise_check as pc
    from fie_amd import hip, mask as hmask
    dt = case[1]
    ctx = hip.context(0, torch.float16 if dt == "f16" else torch.float32)
    dev = ctx.device
    nan = lambda shape, dtype=ctx.dtype: torch.full(shape, float("nan"), device=dev, dtype=dtype)
    if case[0] == "prep":
        _, _, entry, hw, copies = case
        c, mask = _prep_inputs(dt, hw)
        lat, model_in = nan((hw, 4), torch.float32), nan((copies, hw, 8))
        z0 = None if entry[0] == "plain" else nan((hw, 4), torch.float32)
        head = (c["mom"].to(dev), c["eps"].to(dev), c["noise"].to(dev), hw, c["sf"], c["sab"], c["s1mab"], lat, model_in)
        if entry[0] == "plain":
            ctx.latent_prep(*head)
        elif entry[0] == "src":
            ctx.latent_prep_src(*head, z0)
        else:
            ctx.latent_prep_src_content(*head, z0, mask.to(dev), hmask.CONTENT_MODES[entry[1]])
        return _digest((("latents", lat), ("model_in", model_in), ("z0", z0)))
    _, _, fl, hw, nb, ld_eps, last, (want_in, want_dec, copies), scalars = case
    c, z0, n_init, masks, levels = _lcm_inputs(dt, hw, nb, ld_eps)
    s = pc.lcm_scalar_sets()[scalars]
    lat = c["lat"].to(dev)
    model_in = nan((copies, hw, 8)) if want_in else None
    decode_in = nan((1, hw, 8)) if want_dec else None
    head = (c["eps"].to(dev), nb, s["guidance"], lat, None if last else c["noise"].to(dev), hw, s["sab_t"], s["s1mab_t"], s["c_skip"], s["c_out"],
            s["sab_p"], s["s1mab_p"], model_in, s["inv_sf"], decode_in)
    if fl[0] == "plain":
        ctx.lcm_step(*head)
    elif fl[0] == "masked":
        ctx.lcm_step_masked(*head, masks[fl[1]].to(dev), z0.to(dev), n_init.to(dev))
    else:
        ctx.lcm_step_levels(*head, levels.to(dev), z0.to(dev), n_init.to(dev), fl[1], fl[2])
    return _digest((("latents", lat), ("model_in", model_in), ("decode_in", decode_in)))


def differing(a, b):
    """Case keys whose digests differ or that only one side has."""
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="write {case: digest} of this process's library here")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    args = ap.parse_args()
    if args.compare:
        a, b = (json.load(open(p)) for p in args.compare)
        bad = differing(a, b)
        print(f"{len(a)} / {len(b)} cases, " + ("all equal" if not bad else f"{len(bad)} differ:"))
        for k in bad:
            print("   ", k)
        sys.exit(1 if bad else 0)
    if not args.out:
        ap.error("--out or --compare")
    import fie_amd  # noqa: F401
    from fie_amd import hip
    digests = {str(c): run_case(c) for c in cases()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} cases on {hip.LIB_PATH} -> {args.out}")


if __name__ == "__main__":
    main()
