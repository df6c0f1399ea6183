#!/usr/bin/env python3
"""The distinct GEMM / 3x3-conv problems one edit hands the launch table, per product configuration -> tests/golden/launch_problems.json.

    python3 tools/launch_problems.py --out tests/golden/launch_problems.json

Like tools/shape_profile.py::run: eager, ONE stream, no graphs, with the library's launch log on (include/fie.h: fie_debug_oplog), and with
fie_debug_tune_candidates on, so every launch the tuner could decide runs the built-in rule (shapes, not choices: nothing is timed).  Each
configuration runs in a child process of its own (fresh context, its own weights):

  ssd1b_cn      SSD-1B + ControlNet-full, fp16, 1024^2, CFG (BASELINE config 2, the bench line)
  sdxl_b8       SDXL-base + ControlNet-full at batch 8 (config 3: edit_batch of 8 images)
  sdxl_w8       SDXL with fp8 e4m3 weights, fp16 activations (FIE_A8=0)
  sdxl_w8a8     SDXL with fp8 weights and calibrated fp8 activations (config 5)

UNet, ControlNet, CLIP and VAE encode / decode all go through the launch table and are all recorded.  One record per distinct problem: what
it takes to rebuild the call (geometry, side inputs, precision, epilogue; the " | ..." part of a FIE_DESC line, csrc/gemm_conv.hip: run_code),
the rule's tile code, the configurations it appears in and its launch count per configuration.  LayerNorm-folded GEMMs (ln=1) and
GroupNorm-applied halo convs (gna=1) never reach the tuner: recorded with in_scope false."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "ssd1b_cn": dict(model="ssd-1b", weights="f16", batch=1, env={}),
    "sdxl_b8": dict(model="sdxl", weights="f16", batch=8, env={}),
    "sdxl_w8": dict(model="sdxl", weights="f8e4m3", batch=1, env={"FIE_A8": "0"}),
    "sdxl_w8a8": dict(model="sdxl", weights="f8e4m3", batch=1, env={"FIE_A8": "1"}),
}
# the fields of a record that identify a problem (everything but the tile code); the order is the JSON's
FIELDS = ("kind", "M", "N", "K", "K1", "H", "W", "Cin", "stride", "ups", "b", "pad", "C2", "C3", "parity", "w8", "bias", "rowbias", "rpb", "res",
          "act", "scale", "gn", "gnrows", "f8out", "ln", "gna")
_DESC = re.compile(r"^(gemm|conv) M=(\d+) N=(\d+) K=(\d+)(?: in=(\d+)x(\d+)x(\d+) s(\d+) u(\d+))?.* code=(\d+) flop=\S+ \| (.*)$")


def parse_desc(desc):
    """One FIE_DESC line of a GEMM / conv launch -> (problem dict, code), or None for other ops."""
    m = _DESC.match(desc)
    if not m:
        return None
    g = m.groups()
    p = {"kind": g[0], "M": int(g[1]), "N": int(g[2]), "K": int(g[3]),
         "H": int(g[4] or 0), "W": int(g[5] or 0), "Cin": int(g[6] or 0), "stride": int(g[7] or 0), "ups": int(g[8] or 0)}
    for tok in g[10].split():
        k, v = tok.split("=")
        p[k] = float(v) if k == "scale" else int(v)
    return p, int(g[9])


def tune_key(p):
    """The problem's key in the tuner's table (csrc/gemm_conv.hip: fie_tune_key; the format of fie_gemm_autotune_report).  M of a parity conv is the
    per-parity row count, the oplog's M counts all four parities."""
    if p["kind"] == "gemm":
        return f"gemm M={p['M']} N={p['N']} K={p['K']} K1={p['K1']} geom=0 w8={p['w8']}"
    geom = p["stride"] * 2 + p["ups"] + 8 * p["parity"] + 16 * (p["C2"] > 0) + 32 * (p["C3"] > 0)
    m = p["M"] // 4 if p["parity"] else p["M"]
    return f"conv M={m} N={p['N']} K={p['K']} K1={p['K1']} geom={geom} w8={p['w8']}"


def record_one(name, raw_out):
    """Child process: one edit of configuration `name`, logged; writes [[problem, rule code, candidates], ...] in launch order."""
    cfg = CONFIGS[name]
    import fie_amd  # noqa: F401
    import torch
    from bench import synth_item_image
    from src.pipeline import FastEditor
    ed = FastEditor(model_name=cfg["model"], use_full_controlnet=True, enable_cpu_offload=False, weight_dtype=cfg["weights"])
    pipe, ctx = ed.pipe, ed.pipe.ctx
    pipe.fork_streams = False
    pipe.use_graph = False
    ctx.autotune(0)
    imgs = [synth_item_image(3 + i).resize((1024, 1024)) for i in range(cfg["batch"])]
    ctrls = [ed.preprocess_image(im) for im in imgs]
    prompt = "a photo of a [red] house"
    if cfg["weights"] == "f8e4m3" and ctx.a8:
        ed.calibrate_fp8(imgs[0], prompt, strength=0.5, guidance_scale=1.5)      # calibrated activation scales, as bench.py runs config 5
    gen = lambda: torch.Generator().manual_seed(42)
    if cfg["batch"] == 1:
        job = pipe.prepare(prompt, "", imgs[0], ctrls[0], 0.5, 4, 1.5, 0.5, gen())
    else:
        job = pipe.prepare_batch([prompt] * cfg["batch"], [""] * cfg["batch"], imgs, ctrls, 0.5, 4, 1.5, 0.5, [gen() for _ in imgs])
    ctx.tune_candidates(True)
    ctx.oplog(True)
    pipe.run_device(job)
    torch.cuda.synchronize()
    lines = ctx.oplog_read()
    cands = ctx.tune_candidates_read()
    ctx.oplog(False)
    ctx.tune_candidates(False)
    out, ci = [], 0
    for line in lines:
        if line.startswith("#"):
            continue
        parsed = parse_desc(line.split("|", 4)[4])
        if parsed is None:
            continue
        p, code = parsed
        rule, cl = code, None
        if not (p["ln"] or p["gna"]):            # every launch the tuner could decide left one candidates line, in launch order
            key, rule, cl = cands[ci]
            ci += 1
            assert key == tune_key(p), f"candidate line {key!r} does not pair with launch {line!r}"
        out.append([p, rule, cl])
    assert ci == len(cands), f"{len(cands) - ci} candidate lines without a launch"
    with open(raw_out, "w") as f:
        json.dump(out, f)
    print(f"[{name}] {len(out)} GEMM / conv launches, {len(cands)} tunable", flush=True)


def merge(per_config):
    """{config: [[problem, rule, cands], ...]} -> the fixture's records (distinct problems, launch counts per configuration)."""
    recs = {}
    for name, launches in per_config.items():
        for p, rule, cands in launches:
            ident = tuple(p[k] for k in FIELDS)
            r = recs.get(ident)
            if r is None:
                r = recs[ident] = {**{k: p[k] for k in FIELDS}, "key": tune_key(p), "rule": rule, "in_scope": not (p["ln"] or p["gna"]),
                                   "cands_recorded": cands, "configs": {}}
            r["configs"][name] = r["configs"].get(name, 0) + 1
    return sorted(recs.values(), key=lambda r: (r["kind"], r["w8"], r["M"], r["N"], r["K"], r["key"], json.dumps(r, sort_keys=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_problems.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--raw", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        record_one(args.child, args.raw)
        return
    per = {}
    tmp = tempfile.mkdtemp(prefix="launch_problems_")
    for name in args.configs.split(","):
        raw = os.path.join(tmp, f"{name}.json")
        env = {**os.environ, **CONFIGS[name]["env"], "FIE_TUNE_TABLE": os.path.join(ROOT, "tests", "golden", "tune_table.txt"), "FIE_TUNE_FROZEN": "1"}
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--raw", raw], env=env, cwd=ROOT)
        if r.returncode != 0:                    # a failed child ends the run: nothing more is started on the GPU
            sys.exit(f"[{name}] child exited with {r.returncode}")
        print(f"[{name}] {time.time() - t0:.0f} s", flush=True)
        per[name] = json.load(open(raw))
    recs = merge(per)
    doc = {"what": "distinct GEMM / 3x3-conv problems of one edit per configuration (tools/launch_problems.py)",
           "configs": {n: {k: v for k, v in CONFIGS[n].items()} for n in per}, "fields": list(FIELDS), "problems": recs}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=False)
        f.write("\n")
    print(f"{len(recs)} problems ({sum(r['in_scope'] for r in recs)} in scope) -> {args.out}")


if __name__ == "__main__":
    main()
