"""ctypes binding of ``csrc/libfie_hip.so`` (C ABI: include/fie.h) + thin tensor-level wrappers.

PyTorch-ROCm is plumbing here: it owns device memory (``tensor.data_ptr()``) and the current stream; every
multiply-add of the hot path runs in the hand-written HIP kernels behind these wrappers.  There is NO fallback:
if the library is missing or the device is not gfx950 the first call raises.
"""
import ctypes
import numbers
import os
import subprocess

import torch

from . import header

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.environ.get("FIE_LIB_PATH") or os.path.join(_CSRC, "libfie_hip.so")      # FIE_LIB_PATH: A/B builds of the same sources (tools/)

_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float

# include/fie.h is the one statement of the ABI (fie_amd/header.py reads it): the FIE_ACT_* codes, name -> argtypes of every declared function
# (out-pointers are c_void_p: byref(), string buffers and ctypes arrays all pass), the return types and the config structs below
ACT_NONE, ACT_SILU, ACT_GELU, ACT_QUICK_GELU, ACT_GEGLU = (header.DEFINES["ACT_" + n] for n in ("NONE", "SILU", "GELU", "QUICK_GELU", "GEGLU"))
ACT_RELU = header.DEFINES["ACT_RELU"]                  # the fp32 entries only (gemm_f32 / conv3x3_f32: the LPIPS tower)
SIGNATURES = {name: args for name, (_, args) in header.FUNCTIONS.items()}

_lib = None


def build(force=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", _CSRC, "clean"], check=True, capture_output=True)
    r = subprocess.run(["make", "-C", _CSRC, "-j4"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libfie_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no non-HIP fallback for the hot path)")
        _lib = ctypes.CDLL(LIB_PATH)
        for name, (ret, args) in header.FUNCTIONS.items():
            fn = getattr(_lib, name)
            fn.argtypes, fn.restype = args, ret
    return _lib


def last_gemm_kernel(ctx=None):
    """Kernel / tile the last GEMM or conv launch of `ctx` used (names the roofline kernel in bench.py)."""
    ctx = ctx or context(torch.cuda.current_device())
    return lib().fie_debug_last_gemm_kernel(ctx.h).decode()


class FieError(RuntimeError):
    pass


def fold_layernorm_tables(w, bias, gamma, beta, geglu=False):
    """LayerNorm folded into the Linear that consumes it:  LN(x) W^T + b = rstd * (x Wf^T - mean * S) + b'  with Wf = f16(W * gamma), S[n] = sum_k Wf[n, k]
    (over the ROUNDED folded weights, so that x Wf^T - mean * S is exactly (x - mean) Wf^T), b' = W beta + b.  Both are summed in float64 and rounded
    once to fp32: the kernel multiplies S by the row mean, and an S a few fp32 ulps off costs, at a row offset of 300 sigma, what the kernel's whole fp32
    budget is (tests/test_host_cpu.py, profiles/ln_fold_pins.md).  Returns (Wf [N, K] f16,
    table [N, 2] fp32 = (S, b')), the table's rows in the packed column order (GEGLU: value / gate rows interleaved, as fie_pack_rows_f16 with interleave2)."""
    w = w.float()
    n = w.shape[0]
    wf = (w * gamma.float()[None, :]).to(torch.float16)
    b = w.double() @ beta.double()
    if bias is not None:
        b = b + bias.double()
    tab = torch.stack([wf.double().sum(1), b], 1).float()
    if geglu:
        tab = torch.stack([tab[: n // 2], tab[n // 2:]], 1).reshape(n, 2)
    return wf, tab.contiguous()


def _chk(rc):
    if rc != 0:
        raise FieError(f"libfie_hip error {rc}: {lib().fie_last_error().decode()}")


def _p(t):
    return None if t is None else t.data_ptr()


GRAPH_NAMES = ("unet_forward", "controlnet_forward", "vae_encode", "vae_decode", "clip_text_forward")


class VaeConfig(ctypes.Structure):
    """include/fie.h: fie_vae_config (the C++ decoder walk, csrc/graphs.cpp)."""
    _fields_ = header.STRUCTS["fie_vae_config"]


class ClipConfig(ctypes.Structure):
    """include/fie.h: fie_clip_config."""
    _fields_ = header.STRUCTS["fie_clip_config"]


class UnetConfig(ctypes.Structure):
    """include/fie.h: fie_unet_config (UNet and ControlNet)."""
    _fields_ = header.STRUCTS["fie_unet_config"]


class ControlTable(ctypes.Structure):
    """include/fie.h: fie_control_table (the segments of one fie_control_add launch)."""
    _fields_ = header.STRUCTS["fie_control_table"]


class Program:
    """A recorded launch program (include/fie.h, fie_program_*).  `keep` holds every tensor the op wrappers allocated while it
    was recorded: the program references their memory by raw pointer."""

    def __init__(self, ctx):
        self.ctx, self.h, self.keep, self.outputs = ctx, _P(), [], None

    def __len__(self):
        return lib().fie_program_launches(self.h)

    def run(self):
        """Re-issues the launches on torch's current stream.  Ordered against the program's own previous pass by the library (include/fie.h,
        ORDERING CONTRACT); the producers of the static inputs are the caller's to order (`stream.wait_stream(...)`)."""
        self.ctx.sync_stream()
        _chk(lib().fie_program_run(self.ctx.h, self.h))
        return self.outputs

    def register(self, name):
        """Bind to one of the graph-level C entries (fie_unet_forward, ...); `run_named(name)` then calls THAT entry."""
        assert name in GRAPH_NAMES, name
        _chk(lib().fie_graph_register(self.ctx.h, name.encode(), self.h))

    def close(self):
        if self.h:
            lib().fie_program_destroy(self.ctx.h, self.h)
            self.h = _P()


class W8:
    """A packed fp8 (e4m3) weight: bytes [Npad, Kpad] + one fp32 dequantisation scale per output channel (include/fie.h,
    fie_pack_*_f8).  `stride(0)` mirrors the packed fp16 tensors so call sites stay the same."""

    def __init__(self, q, scale):
        self.q, self.scale = q, scale

    def stride(self, d):
        return self.q.stride(d)

    def dequant(self):
        return self.q.view(torch.float8_e4m3fn).float() * self.scale[:, None]


class Context:
    """One fie_ctx per (process, device); launches go to torch's current stream on that device."""

    def __init__(self, device=0, dtype=torch.float16):
        if dtype not in (torch.float16, torch.float32):
            raise ValueError(f"dtype {dtype} not supported (float16 or float32)")
        self.dtype = dtype                           # storage / arithmetic type of every op issued through this context
        self.f32 = dtype == torch.float32
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: the fie_amd hot path has no CPU fallback")
        self.device = torch.device("cuda", device)
        h = _P()
        _chk(lib().fie_ctx_create(device, None, ctypes.byref(h)))
        self.h = h
        # device error word (include/fie.h: FIE_DEVERR_*): kernels that must give up set it; check_device_errors() reads it
        self._err = torch.zeros(4, device=self.device, dtype=torch.int32)
        self._err_host = torch.zeros(4, dtype=torch.int32).pin_memory()
        _chk(lib().fie_ctx_error_flag(self.h, self._err.data_ptr()))
        self._stream = None
        self._gn_ws = {}
        self._gn_stats = {}
        self._ws_retired = []          # scratch buffers a larger one has replaced (_scratch): a captured hipGraph may still hold their address
        self._gn_gen = 0
        self._sk_ws = {}               # split-K workspaces (fie_splitk_workspace), one per (stream, graph slot)
        self._sk_bound = None
        self._sk_pinned = False        # True while a program records: the program's OWN workspace stays bound (record())
        self._cap_stream = None
        self._prog_ws = []             # weak references to the live programs' workspaces (splitk_counters_clear)
        self.splitk_bytes = int(os.environ.get("FIE_SPLITK_MB", "96")) << 20      # 0: never split K
        self.gn_from_epilogue = os.environ.get("FIE_GN_FROM_EPILOGUE", "1") != "0"
        self.gn_quads = os.environ.get("FIE_GN_QUADS", "1") != "0"      # ... also for the UNet's 20 / 40-channel groups (quad partials); A/B switch
        self._epi_prefetch = True                 # C side default (fie_debug_epilogue_prefetch)
        self.up2x_parity = os.environ.get("FIE_UP2X_PARITY", "1") != "0"
        # transformer blocks: LayerNorm folded into the projection that consumes it (fie_gemm_ln_f16: no LayerNorm launch, no normalised tensor); A/B switch
        self.ln_fold = os.environ.get("FIE_LN_FOLD", "1") != "0"
        # ... also norm3 -> the GEGLU projection (256x320 tile): built and bit-checked, but the row sums add 11-15 us to a 49 us launch there (every wave of a
        # wave row sums the same fragments; dealing them out needs branches in the K loop, which cost as much): off, LayerNorm launch + plain FF1
        self.kv_group = os.environ.get("FIE_KV_GROUP", "1") != "0"      # text K/V of all transformer blocks of a net as one GEMM per image (nn.py: _finish_kv); A/B switch
        self.ln_fold_which = os.environ.get("FIE_LN_FOLD_WHICH", "qkv,q2")      # which of the two folds run (A/B)
        self.ln_fold_ff1 = os.environ.get("FIE_LN_FOLD_FF1", "0") != "0"
        self.conv_plus_shortcut = os.environ.get("FIE_CONV_PLUS", "1") != "0"   # resnet conv2 + 1x1 shortcut as one GEMM (fie_conv3x3_plus_nhwc_f16)      # 2x-upsampling convs as four 2x2 convs (fie_conv_up2x_nhwc_f16)
        self._resize_tables = {}       # (in, out) -> (taps, bounds, ksize) of the LANCZOS resample, on the device; ("bicubic", in, out) likewise; ("nearest", in, out) -> indices
        self.ws_tag = 0
        self._keep = None              # list collecting the tensors allocated while a program is being recorded (Context.record)
        self.w8 = False                # while True, pack_linear / pack_conv3x3 quantise eligible weights to fp8 e4m3 (see W8)
        # fp8 ACTIVATIONS for the transformer-block projections of an fp8-weight model (csrc/gemm_x8.hip): the producers (LayerNorm, attention,
        # the GEGLU epilogue) write e4m3 and the GEMMs run the block-scaled MFMA.  FIE_A8=0 keeps fp16 activations (round-2 behaviour: A/B)
        self.a8 = os.environ.get("FIE_A8", "1") != "0"
        # GroupNorm + SiLU applied by the consuming halo conv (conv3x3_gn): built, bit-exact, and 20-70 % SLOWER than the two launches (the transform's
        # exp / rcp do not fit the issue slots the MFMA segments leave: profiles/r04_gn_apply_in_the_halo_conv_negative.log) -- off unless FIE_GN_FUSE_CONV=1
        self.gn_fuse_conv = os.environ.get("FIE_GN_FUSE_CONV", "0") == "1"
        self.calib = False             # True during HipImg2ImgPipeline.calibrate_fp8: fp8-activation layers run f16 activations and record max |x|
        # Tile / split-K choices from a file (include/fie.h: fie_gemm_autotune_load): FIE_TUNE_TABLE=<report of an earlier process>.  With
        # FIE_TUNE_FROZEN=1 the pipelines never time anything new (shapes outside the table use the built-in rule): one choice per shape on
        # every box, which is what the test session pins (tests/conftest.py); direct ctx.autotune(1) calls still tune live.
        self.tune_frozen = os.environ.get("FIE_TUNE_FROZEN", "0") == "1"
        self.tune_table_entries = 0
        self.load_tune_table()

    def fetch_device_errors(self):
        """Queues the 16-byte D2H copy of the error word on the current stream (call before a synchronisation that happens anyway)."""
        self._err_host.copy_(self._err, non_blocking=True)

    def check_device_errors(self, fetch=True):
        """Raises FieError when a kernel reported a device-side failure since the last check (clears the word)."""
        if fetch:
            self.fetch_device_errors()
            torch.cuda.current_stream(self.device).synchronize()
        code = int(self._err_host[0])
        if code:
            self._err.zero_()
            self._err_host.zero_()
            what = {1: "fie_time_embed_f16: the in-launch barrier timed out (a workgroup never arrived); the timestep embedding of that "
                       "launch is invalid"}.get(code, "unknown device error")
            raise FieError(f"device error {code}: {what}")

    def sync_stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream:
            _chk(lib().fie_ctx_set_stream(self.h, s))
            self._stream = s

    def load_tune_table(self, path=None):
        """Remembered tile / split-K choices from the text of an autotune report (FIE_TUNE_TABLE by default).  Returns the number loaded."""
        path = path or os.environ.get("FIE_TUNE_TABLE")
        if not path or self.f32:
            return 0
        with open(path) as f:
            n = lib().fie_gemm_autotune_load(self.h, f.read().encode())
        if n < 0:
            raise FieError(f"fie_gemm_autotune_load: {lib().fie_last_error().decode()}")
        self.tune_table_entries = n
        return n

    def _bind_splitk(self):
        """Split-K launches that may run concurrently must not share arrival counters / slabs: every (stream, graph slot) owns a
        workspace (zeroed once: the kernels leave the counters zero), bound to the C context before a GEMM / conv or a C++ graph walk is
        issued there.  While a program records, the program's own workspace stays bound instead (record())."""
        if self._sk_pinned or self.f32 or not self.splitk_bytes:
            return
        key = (self._stream, self.ws_tag)
        if key == self._sk_bound:
            return
        ws = self._sk_ws.get(key)
        if ws is None:
            # under stream capture torch.zeros would become a 96 MB memset node replayed with the graph: callers that capture bind the capture
            # stream's workspace BEFORE entering the capture (pipe._capture); a key first met inside a capture keeps working, only slower
            ws = self._sk_ws[key] = torch.zeros(self.splitk_bytes, device=self.device, dtype=torch.uint8)
        _chk(lib().fie_splitk_workspace(self.h, ws.data_ptr(), ws.numel()))
        self._sk_bound = key

    def capture_stream(self):
        """The stream this context's hipGraph captures run on (`torch.cuda.graph(g, stream=ctx.capture_stream())`), with the split-K workspace
        of (that stream, current ws_tag) bound BEFORE the capture begins: allocated inside a capture, its torch.zeros would be a 96 MB memset
        node that every replay re-runs."""
        if self._cap_stream is None:
            self._cap_stream = torch.cuda.Stream(device=self.device)
        with torch.cuda.stream(self._cap_stream):
            self.sync_stream()
            self._bind_splitk()
        torch.cuda.synchronize(self.device)
        return self._cap_stream

    def splitk_counters_clear(self):
        """True when every arrival counter of every split-K workspace of this context is zero (synchronises): what each launch must leave."""
        torch.cuda.synchronize(self.device)
        live = list(self._sk_ws.values()) + [w for w in (r() for r in self._prog_ws) if w is not None]
        return all(int(ws[:16384].view(torch.int32).abs().max()) == 0 for ws in live)

    # ------------------------------------------------------------------ launch programs / graph-level entries
    def record(self):
        """Context manager: `with ctx.record() as prog: out = model(...)` executes the ops as usual AND records every launch into
        `prog`.  Works on whatever torch stream is current; tensors allocated by the op wrappers meanwhile stay referenced by
        `prog.keep` (torch must not hand their memory to anybody else while the program lives)."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            prog = Program(self)
            self.sync_stream()
            # the program OWNS its split-K workspace (include/fie.h, ORDERING CONTRACT (2)): the recorded launches freeze its pointer, and no
            # stream's eager launches or other program ever share its arrival counters / slabs
            own = None
            if not self.f32 and self.splitk_bytes:
                own = torch.zeros(self.splitk_bytes, device=self.device, dtype=torch.uint8)
                prog.keep.append(own)
                import weakref
                self._prog_ws = [r for r in self._prog_ws if r() is not None] + [weakref.ref(own)]
                _chk(lib().fie_splitk_workspace(self.h, own.data_ptr(), own.numel()))
                self._sk_pinned = True
            _chk(lib().fie_program_begin(self.h, ctypes.byref(prog.h)))
            self._keep = prog.keep
            try:
                yield prog
            finally:
                self._keep = None
                _chk(lib().fie_program_end(self.h))
                if own is not None:
                    self._sk_pinned = False
                    self._sk_bound = None           # the next GEMM / conv re-binds its stream's workspace
        return cm()

    def run_named(self, name):
        """Run the program registered under `name` through its C-ABI graph entry (fie_unet_forward, fie_vae_decode, ...)."""
        self.sync_stream()
        _chk(getattr(lib(), "fie_" + name)(self.h))

    def _scratch(self, cache, key, need):
        """cache[key] when it holds `need` bytes, else a new u8 buffer of that size in its place.  The buffer it replaces is NOT freed: a hipGraph
        captured on that (stream, graph slot) has its address in its launches, and a later replay would write into whatever torch has put there
        since -- or, once a capture's empty_cache() has returned the block to the driver, into an unmapped page.  (An edit of three images after
        an edit of one grows the GroupNorm scratch of the ControlNet's side stream; replaying the first edit's graph afterwards faulted.)  The
        sizes follow the batch and the map and each replacement is larger than the last, so what is kept stays below the live buffers' size."""
        buf = cache.get(key)
        if buf is None or buf.numel() < need:
            if buf is not None:
                self._ws_retired.append(buf)
            buf = cache[key] = torch.empty(need, device=self.device, dtype=torch.uint8)
        return buf

    def _alloc(self, shape, dtype=None, zero=False):
        t = (torch.zeros if zero else torch.empty)(shape, device=self.device, dtype=dtype or self.dtype)
        if self._keep is not None:
            self._keep.append(t)
        return t

    # ------------------------------------------------------------------ tuning / test hooks (per ctx)
    def force_tile(self, code):
        """0 = heuristic; see include/fie.h for the codes.  An ineligible code makes the op raise FieError."""
        _chk(lib().fie_debug_force_tile(self.h, int(code)))

    def prefetch(self, t, stream=None, blocks=16):
        """Pull tensor t (a packed weight) into the Infinity Cache on `stream` (a torch stream; default: the context's)."""
        _chk(lib().fie_prefetch(self.h, t.data_ptr(), t.numel() * t.element_size(), stream.cuda_stream if stream is not None else None, int(blocks)))

    def autotune(self, on=True):
        """Per-shape tile autotune (include/fie.h: fie_gemm_autotune): first eager launch of a shape times the eligible tiles."""
        _chk(lib().fie_gemm_autotune(self.h, int(on)))                # 0 off, 1 tune new shapes, 2 remembered shapes only

    def tune_exclude(self, codes):
        """Tile codes ("63,96"; 10000 = all split-K variants) the tuner must not offer; forgets remembered choices (A/B tools)."""
        return lib().fie_debug_tune_exclude(self.h, (codes or "").encode())

    def autotune_report(self):
        buf = ctypes.create_string_buffer(1 << 20)
        n = lib().fie_gemm_autotune_report(self.h, buf, len(buf))
        return n, buf.value.decode()

    def splitk(self, on=True):
        """False: no launch of this context splits K (A/B switch; the tuner's remembered split choices fall back to the unsplit tile)."""
        _chk(lib().fie_debug_splitk(self.h, int(bool(on))))

    def oplog(self, on=True):
        """Launch log (include/fie.h: fie_debug_oplog): one line per kernel launch with the op's shape description."""
        _chk(lib().fie_debug_oplog(self.h, int(on)))
        self._oplog_on = bool(on)

    def oplog_mark(self, text):
        if getattr(self, "_oplog_on", False):
            _chk(lib().fie_debug_oplog_mark(self.h, text.encode()))

    def oplog_read(self):
        n = lib().fie_debug_oplog_read(self.h, None, 0)
        buf = ctypes.create_string_buffer(int(n) + 16)
        lib().fie_debug_oplog_read(self.h, buf, len(buf))
        return [l for l in buf.value.decode().split("\n") if l]

    def tune_candidates(self, on=True):
        """While on, GEMM / conv launches the tuner could decide run the rule's code and report what the tuner would time (include/fie.h:
        fie_debug_tune_candidates); tune_candidates_read() returns [(key, rule, [candidates])], key in the format of autotune_report."""
        _chk(lib().fie_debug_tune_candidates(self.h, int(on)))

    def tune_candidates_read(self):
        n = lib().fie_debug_tune_candidates_read(self.h, None, 0)
        buf = ctypes.create_string_buffer(int(n) + 16)
        lib().fie_debug_tune_candidates_read(self.h, buf, len(buf))
        out = []
        for line in buf.value.decode().split("\n"):
            if line:
                key, rest = line.split(" rule=")
                rule, cands = rest.split(" cands=")
                out.append((key, int(rule), [int(c) for c in cands.split(",") if c]))
        return out

    def gemm_stamps(self, buf):
        """Device int32 tensor [tiles * waves * 8] the stamped ring kernels (tile codes 97 / 98) write their cycle sums to; None detaches."""
        _chk(lib().fie_debug_gemm_stamps(self.h, buf.data_ptr() if buf is not None else None))

    def gemm_probe(self, mode):
        """TIMING-ONLY probes of the LDS-DMA GEMM kernels (outputs are wrong): 0 off, 1 loads dropped, 2 all tiles load tile (0,0)."""
        _chk(lib().fie_debug_gemm_probe(self.h, int(mode)))

    @property
    def epi_prefetch(self):
        return self._epi_prefetch

    @epi_prefetch.setter
    def epi_prefetch(self, on):
        """A/B switch: bias row / residual tile of the ring GEMM and conv kernels loaded ahead of the K loop (default) or in the epilogue."""
        _chk(lib().fie_debug_epilogue_prefetch(self.h, int(bool(on))))
        self._epi_prefetch = bool(on)

    def tile_override(self, spec):
        """"mode,M,N,K=code;..." per-shape tile codes (None clears).  Returns the number of entries parsed."""
        return lib().fie_debug_tile_override(self.h, spec.encode() if spec else None)

    def close(self):
        if self.h:
            lib().fie_ctx_destroy(self.h)
            self.h = None

    # ------------------------------------------------------------------ weight packing
    def pack_linear(self, w, geglu=False, quant=True):
        """[N, K] f16 -> packed [Npad][Kpad] (zero padded); geglu interleaves (value, gate) rows.
        fp32 contexts keep plain [N, K] fp32 weights (rows interleaved for GEGLU)."""
        self.sync_stream()
        if self.f32:
            w = w.to(self.device, torch.float32)
            if geglu:
                n = w.shape[0]
                w = torch.stack([w[: n // 2], w[n // 2:]], 1).reshape(n, -1)
            return w.contiguous()
        w = w.to(self.device, torch.float16).contiguous()
        n, k = w.shape
        npad, kpad = (n + 127) // 128 * 128, (k + 63) // 64 * 64
        if self.w8 and quant and self.a8:
            kpad = (k + 127) // 128 * 128               # the fp8-activation kernels step K by 128
        if self.w8 and quant:
            q = torch.empty((npad, kpad), device=self.device, dtype=torch.uint8)
            scale = torch.empty((npad,), device=self.device, dtype=torch.float32)
            _chk(lib().fie_pack_rows_f8(self.h, _p(w), k, n, k, _p(q), kpad, npad, _p(scale), int(geglu)))
            return W8(q, scale)
        out = torch.empty((npad, kpad), device=self.device, dtype=torch.float16)
        _chk(lib().fie_pack_rows_f16(self.h, _p(w), k, n, k, _p(out), kpad, npad, int(geglu)))
        return out

    def pack_conv3x3(self, w, cin_pad=None, quant=True):
        """OIHW f16 -> packed [Npad][Kpad], k = (ky*3+kx)*cin_pad + ci.  fp32 contexts: [Cout][9*cin_pad] fp32."""
        self.sync_stream()
        if self.f32:
            co, ci = w.shape[:2]
            cp = cin_pad or (ci + 7) // 8 * 8
            out = torch.zeros((co, 3, 3, cp), device=self.device, dtype=torch.float32)
            out[..., :ci] = w.to(self.device, torch.float32).permute(0, 2, 3, 1)
            return out.reshape(co, 9 * cp)
        w = w.to(self.device, torch.float16).contiguous()
        co, ci = w.shape[:2]
        cin_pad = cin_pad or (ci + 7) // 8 * 8
        npad, kpad = (co + 127) // 128 * 128, (9 * cin_pad + 63) // 64 * 64
        if self.w8 and quant and cin_pad % 64 == 0:  # the fp8 kernels are the LDS-DMA ones: K-steps must not straddle a 3x3 tap
            q = torch.empty((npad, kpad), device=self.device, dtype=torch.uint8)
            scale = torch.empty((npad,), device=self.device, dtype=torch.float32)
            _chk(lib().fie_pack_conv3x3_f8(self.h, _p(w), co, ci, cin_pad, _p(q), kpad, npad, _p(scale)))
            return W8(q, scale)
        out = torch.empty((npad, kpad), device=self.device, dtype=torch.float16)
        _chk(lib().fie_pack_conv3x3_f16(self.h, _p(w), co, ci, cin_pad, _p(out), kpad, npad))
        return out

    # ------------------------------------------------------------------ ops
    # ---- GroupNorm statistics from the producing GEMM / conv (include/fie.h: fie_gn_stats_target)
    def _gn_stats_arm(self, rows_total, n, rows_per_image, groups):
        """Arms the next launch to write GroupNorm partial sums of its [rows_total, n] output; returns the tag groupnorm() looks for on
        the output tensor, or None when the shape is not eligible (channels per group not 4 / 8 / 16, rows not in 32-row granules)."""
        if not self.gn_from_epilogue or self.f32 or not groups or n % groups:
            return None
        if rows_per_image % 32 or rows_total % rows_per_image:
            return None
        cg, pgroups = n // groups, groups
        if cg not in (4, 8, 16):
            # the UNet's 20 / 40-channel groups: the producer writes one slot per 4-channel quad and the consumer sums the quads of a group.
            # Only where the three-kernel GroupNorm would run (64x64 latents and up): the small maps take the single-pass kernel, one launch
            if cg % 4 or rows_per_image < 4096 or not self.gn_quads:
                return None
            pgroups = n // 4
        b = rows_total // rows_per_image
        need = lib().fie_gn_stats_bytes(b, rows_per_image, pgroups)
        key = (self._stream, self.ws_tag)            # one buffer per stream and graph slot: a producer's sums are consumed before the next producer runs
        buf = self._scratch(self._gn_stats, key, need)
        if self._keep is not None:
            self._keep.append(buf)
        _chk(lib().fie_gn_stats_target(self.h, _p(buf), rows_per_image, pgroups))
        self._gn_gen += 1
        return (buf, groups, n, rows_per_image, b, self._gn_gen, key, pgroups)

    def gemm(self, a, wp, n, out=None, a2=None, bias=None, rowbias=None, rows_per_batch=0, residual=None, scale=1.0,
             act=ACT_NONE, k=None, gn_stats=None, a_scale=1.0, out_f8=False, out_inv_scale=1.0):
        """a: [M, K1] (last-dim contiguous, row stride free), optional a2: [M, K2]; wp packed weight; n logical N.
        a of dtype uint8 = e4m3 activations (fie_gemm_x8_f16; a_scale = their dequantisation scale); out_f8: the output is e4m3 bytes too."""
        self.sync_stream()
        self._bind_splitk()
        m, k1 = a.shape
        ktot = k1 + (a2.shape[1] if a2 is not None else 0)
        if k is not None:
            assert k == ktot
        nout = n // 2 if act == ACT_GEGLU else n
        if out is None:
            out = self._alloc((m, nout), torch.uint8 if out_f8 else None)
        assert a.stride(1) == 1 and out.stride(1) == 1
        if self.f32:
            return self.gemm_f32(a, wp, n, out, a2=a2, bias=bias, rowbias=rowbias, rows_per_batch=rows_per_batch, residual=residual, scale=scale, act=act)
        if a.dtype == torch.uint8:                      # e4m3 activations (written by a producer with out_f8) x e4m3 weights
            assert isinstance(wp, W8) and a2 is None and wp.stride(0) % 128 == 0, "fp8 activations need fp8 weights packed with Kpad % 128 == 0"
            if out_f8 and out.dtype != torch.uint8:
                raise ValueError("out_f8 needs a uint8 output tensor")
            _chk(lib().fie_gemm_x8_f16(self.h, _p(a), a.stride(0), _p(wp.q), wp.stride(0), _p(wp.scale), float(a_scale), _p(out), out.stride(0), m, n, ktot,
                                       _p(bias), _p(rowbias), rowbias.stride(0) if rowbias is not None else 0, rows_per_batch, _p(residual),
                                       residual.stride(0) if residual is not None else 0, float(scale), act, int(out_f8), float(out_inv_scale)))
            return out
        if isinstance(wp, W8):
            _chk(lib().fie_gemm_w8_f16(self.h, _p(a), a.stride(0), k1, _p(a2), a2.stride(0) if a2 is not None else 0,
                                       _p(wp.q), wp.stride(0), _p(wp.scale), _p(out), out.stride(0), m, n, ktot, _p(bias), _p(rowbias),
                                       rowbias.stride(0) if rowbias is not None else 0, rows_per_batch, _p(residual),
                                       residual.stride(0) if residual is not None else 0, float(scale), act))
            return out
        tag = self._gn_stats_arm(m, n, gn_stats[0], gn_stats[1]) if gn_stats and act != ACT_GEGLU and out.stride(0) == n else None
        _chk(lib().fie_gemm_f16(self.h, _p(a), a.stride(0), k1, _p(a2), a2.stride(0) if a2 is not None else 0,
                                _p(wp), wp.stride(0), _p(out), out.stride(0), m, n, ktot, _p(bias), _p(rowbias),
                                rowbias.stride(0) if rowbias is not None else 0, rows_per_batch, _p(residual),
                                residual.stride(0) if residual is not None else 0, float(scale), act))
        out._gn_tag = tag
        return out

    def gemm_f32(self, a, wp, n, out=None, a2=None, bias=None, rowbias=None, rows_per_batch=0, residual=None, scale=1.0, act=ACT_NONE):
        """gemm() on fp32 tensors through fie_gemm_f32, from a context of either dtype (the fp32 context's gemm() is this): a [M, K1] (+ a2 [M, K2])
        f32, wp plain [N, K] f32 weights, out [M, n] f32 (row stride free).  act may be ACT_RELU."""
        self.sync_stream()
        m, k1 = a.shape
        ktot = k1 + (a2.shape[1] if a2 is not None else 0)
        if out is None:
            out = self._alloc((m, n // 2 if act == ACT_GEGLU else n), torch.float32)
        assert a.stride(1) == 1 and out.stride(1) == 1 and a.dtype == torch.float32 and wp.dtype == torch.float32 and out.dtype == torch.float32
        _chk(lib().fie_gemm_f32(self.h, _p(a), a.stride(0), k1, _p(a2), a2.stride(0) if a2 is not None else 0, _p(wp),
                                wp.stride(0), 0, _p(out), out.stride(0), m, n, ktot, _p(bias), _p(rowbias),
                                rowbias.stride(0) if rowbias is not None else 0, rows_per_batch, _p(residual),
                                residual.stride(0) if residual is not None else 0, float(scale), act, 1, 1, 0, 0, 0, 0, 0, 0))
        return out

    def fold_layernorm(self, w, bias, gamma, beta, geglu=False):
        """Prepares a Linear whose input is a LayerNorm for gemm_ln (include/fie.h: fie_gemm_ln_f16): the packed f16 matrix of W * gamma and the fp32 table
        [(sum_k Wf[n, k], (W beta)[n] + bias[n])] in the packed column order (fold_layernorm_tables below: the algebra, device-free)."""
        dev = lambda t: None if t is None else t.to(self.device)
        wf, tab = fold_layernorm_tables(dev(w), dev(bias), dev(gamma), dev(beta), geglu=geglu)
        return self.pack_linear(wf, geglu=geglu, quant=False), tab

    def gemm_ln(self, x, wp, n, tab, eps=1e-5, act=ACT_NONE, out=None):
        """out = act(LayerNorm(x) @ W^T + bias) with the LayerNorm folded into the GEMM (fold_layernorm prepared wp / tab); x: [M, K] un-normalised."""
        self.sync_stream()
        m, k = x.shape
        nout = n // 2 if act == ACT_GEGLU else n
        if out is None:
            out = self._alloc((m, nout))
        assert x.stride(1) == 1 and out.stride(1) == 1 and tab.dtype == torch.float32 and tab.shape == (n, 2) and not self.f32
        _chk(lib().fie_gemm_ln_f16(self.h, _p(x), x.stride(0), _p(wp), wp.stride(0), _p(tab), float(eps), _p(out), out.stride(0), m, n, k, act))
        out._gn_tag = None
        return out

    def conv3x3_plus(self, x, wp, cout, x2, x3=None, bias=None, rowbias=None, scale=1.0, act=ACT_NONE, gn_groups=None, out=None):
        """conv3x3(x) + [x2 | x3] @ W1x1^T in one GEMM (include/fie.h: fie_conv3x3_plus_nhwc_f16); x2 / x3: [B*H*W, C] views, last dim contiguous."""
        self.sync_stream()
        self._bind_splitk()
        b, h, w, cin = x.shape
        assert x.is_contiguous() and not self.f32 and x2.stride(1) == 1 and (x3 is None or x3.stride(1) == 1)
        if out is None:
            out = self._alloc((b, h, w, cout))
        tag = self._gn_stats_arm(b * h * w, cout, h * w, gn_groups) if gn_groups else None
        _chk(lib().fie_conv3x3_plus_nhwc_f16(self.h, _p(x), b, h, w, cin, _p(wp), wp.stride(0), _p(out), out.stride(2), cout, _p(bias), _p(rowbias),
                                             rowbias.stride(0) if rowbias is not None else 0, float(scale), act, _p(x2), x2.stride(0), x2.shape[1],
                                             _p(x3), x3.stride(0) if x3 is not None else 0, x3.shape[1] if x3 is not None else 0))
        out._gn_tag = tag
        return out

    def pack_conv_up2x(self, w):
        """OIHW 3x3 weights -> the four parity matrices of fie_conv_up2x_nhwc_f16, [4][Npad][Kpad] f16: for output parity (py, px) the taps
        that fall on the same input pixel are summed (fp32, rounded once): rows {ky 0} | {ky 1, 2} for parity 0, {ky 0, 1} | {ky 2} for 1."""
        w = w.to(self.device, torch.float32)
        sets = (((0,), (1, 2)), ((0, 1), (2,)))
        mats = []
        for py in range(2):
            for px in range(2):
                taps = [sum(w[:, :, ky, kx] for ky in sets[py][a] for kx in sets[px][b]) for a in range(2) for b in range(2)]    # 4 x [Cout, Cin]
                mats.append(self.pack_linear(torch.stack(taps, 1).reshape(w.shape[0], -1).to(torch.float16), quant=False))
        return torch.stack(mats).contiguous()

    def conv_up2x(self, x, wp4, cout, bias=None, rowbias=None, scale=1.0, act=ACT_NONE, gn_groups=None, out=None):
        """conv3x3(nearest-2x(x)) from the four parity matrices of pack_conv_up2x: x [B, H, W, Cin] -> [B, 2H, 2W, cout]."""
        self.sync_stream()
        self._bind_splitk()
        b, h, w, cin = x.shape
        assert x.is_contiguous() and not self.f32 and cin % 64 == 0
        if out is None:
            out = self._alloc((b, 2 * h, 2 * w, cout))
        tag = self._gn_stats_arm(b * 4 * h * w, cout, 4 * h * w, gn_groups) if gn_groups else None
        _chk(lib().fie_conv_up2x_nhwc_f16(self.h, _p(x), b, h, w, cin, _p(wp4), wp4.stride(1), wp4.shape[1], _p(out), out.stride(2), cout,
                                          _p(bias), _p(rowbias), rowbias.stride(0) if rowbias is not None else 0, float(scale), act))
        out._gn_tag = tag
        return out

    def conv3x3(self, x, wp, cout, out=None, stride=1, pad_mode=0, upsample=False, bias=None, rowbias=None,
                residual=None, scale=1.0, act=ACT_NONE, ldc=None, gn_groups=None, a_scale=1.0):
        """x: [B, H, W, Cin] f16 contiguous NHWC -> [B, OH, OW, ldc]."""
        self.sync_stream()
        self._bind_splitk()
        b, h, w, cin = x.shape
        assert x.is_contiguous()
        hin, win = (h * 2, w * 2) if upsample else (h, w)
        pads = 2 if pad_mode == 0 else 1
        oh, ow = (hin + pads - 3) // stride + 1, (win + pads - 3) // stride + 1
        ldc = ldc or cout
        if out is None:
            out = self._alloc((b, oh, ow, ldc), zero=ldc != cout)
        if x.dtype == torch.uint8:                      # e4m3 activations from a GroupNorm with out_f8 (fie_conv3x3_x8_nhwc_f16)
            assert isinstance(wp, W8) and cin % 128 == 0 and wp.stride(0) % 128 == 0
            tag = self._gn_stats_arm(b * oh * ow, cout, oh * ow, gn_groups) if gn_groups and ldc == cout else None
            _chk(lib().fie_conv3x3_x8_nhwc_f16(self.h, _p(x), b, h, w, cin, int(upsample), stride, pad_mode, _p(wp.q), wp.stride(0), _p(wp.scale), float(a_scale),
                                               _p(out), out.stride(2), cout, _p(bias), _p(rowbias), rowbias.stride(0) if rowbias is not None else 0,
                                               _p(residual), residual.stride(2) if residual is not None else 0, float(scale), act))
            out._gn_tag = tag
            return out
        if isinstance(wp, W8):
            _chk(lib().fie_conv3x3_w8_nhwc_f16(self.h, _p(x), b, h, w, cin, int(upsample), stride, pad_mode, _p(wp.q), wp.stride(0),
                                               _p(wp.scale), _p(out), out.stride(2), cout, _p(bias), _p(rowbias),
                                               rowbias.stride(0) if rowbias is not None else 0, _p(residual),
                                               residual.stride(2) if residual is not None else 0, float(scale), act))
            return out
        if self.f32:
            out = self.conv3x3_f32(x, wp, cout, out, stride=stride, pad_mode=pad_mode, upsample=upsample, bias=bias, rowbias=rowbias, residual=residual,
                                   scale=scale, act=act)
            out._gn_tag = None
            return out
        tag = self._gn_stats_arm(b * oh * ow, cout, oh * ow, gn_groups) if gn_groups and ldc == cout else None
        _chk(lib().fie_conv3x3_nhwc_f16(self.h, _p(x), b, h, w, cin, int(upsample), stride, pad_mode, _p(wp),
                                        wp.stride(0), _p(out), out.stride(2), cout, _p(bias), _p(rowbias),
                                        rowbias.stride(0) if rowbias is not None else 0, _p(residual),
                                        residual.stride(2) if residual is not None else 0, float(scale), act))
        out._gn_tag = tag
        return out

    def conv3x3_f32(self, x, wp, cout, out, stride=1, pad_mode=0, upsample=False, bias=None, rowbias=None, residual=None, scale=1.0, act=ACT_NONE):
        """conv3x3() on fp32 tensors through fie_conv3x3_nhwc_f32, from a context of either dtype (the fp32 context's conv3x3() is this): x [B, H, W, Cin]
        f32 contiguous, wp [cout, 9 Cin] f32 in (ky, kx, ci) order, out a [B, OH, OW, >= cout] f32 tensor or channel range of one (its pixel stride
        is the row stride the op writes with).  act may be ACT_RELU."""
        self.sync_stream()
        b, h, w, cin = x.shape
        assert x.is_contiguous() and x.dtype == torch.float32 and wp.dtype == torch.float32 and out.dtype == torch.float32 and out.stride(3) == 1
        _chk(lib().fie_conv3x3_nhwc_f32(self.h, _p(x), b, h, w, cin, int(upsample), stride, pad_mode, _p(wp),
                                        wp.stride(0), _p(out), out.stride(2), cout, _p(bias), _p(rowbias),
                                        rowbias.stride(0) if rowbias is not None else 0, _p(residual),
                                        residual.stride(2) if residual is not None else 0, float(scale), act))
        return out

    def attention(self, q, k, v, heads, head_dim, tq, tk, batch, out=None, causal=False, scale=None, out_f8=False, out_inv_scale=1.0):
        """q: [B*Tq, >=H*D] view (row stride free); k, v: [B*Tk, ...]; returns [B*Tq, H*D] (out_f8: as e4m3 bytes, value * out_inv_scale)."""
        self.sync_stream()
        if out is None:
            out = self._alloc((batch * tq, heads * head_dim), torch.uint8 if out_f8 else None)
        scale = scale if scale is not None else head_dim ** -0.5
        if self.f32:
            # S = Q K^T (batched over image x head) -> row softmax -> O = P V; the fp32 scores are simply materialised
            s_ = self._alloc((batch * heads, tq, tk), torch.float32)
            d = head_dim
            _chk(lib().fie_gemm_f32(self.h, _p(q), q.stride(0), d, None, 0, _p(k), k.stride(0), 0, _p(s_), tk, tq, tk, d, None, None, 0,
                                    0, None, 0, 1.0, ACT_NONE, batch, heads, tq * q.stride(0), d, tk * k.stride(0), d,
                                    heads * tq * tk, tq * tk))
            _chk(lib().fie_softmax_rows_f32(self.h, _p(s_), batch * heads * tq, tk, tk, float(scale), int(causal), tq))
            _chk(lib().fie_gemm_f32(self.h, _p(s_), tk, tk, None, 0, _p(v), v.stride(0), 1, _p(out), out.stride(0), tq, d, tk, None,
                                    None, 0, 0, None, 0, 1.0, ACT_NONE, batch, heads, heads * tq * tk, tq * tk, tk * v.stride(0), d,
                                    tq * out.stride(0), d))
            return out
        if out_f8:
            _chk(lib().fie_attention_f16_o8(self.h, _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0), batch, heads, tq, tk,
                                            head_dim, float(scale), int(causal), float(out_inv_scale)))
            return out
        _chk(lib().fie_attention_f16(self.h, _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out),
                                     out.stride(0), batch, heads, tq, tk, head_dim, float(scale), int(causal)))
        return out

    def groupnorm(self, x1, gamma, beta, groups, eps, silu, x2=None, out=None, out_f8=False, out_inv_scale=1.0):
        """x1: [B, rows, C1] (+ x2: [B, rows, C2]) NHWC-flattened, contiguous -> [B, rows, C1+C2] (out_f8: as e4m3 bytes, value * out_inv_scale)."""
        self.sync_stream()
        b, rows, c1 = x1.shape[0], x1[0].numel() // x1.shape[-1], x1.shape[-1]
        c2 = x2.shape[-1] if x2 is not None else 0
        assert x1.is_contiguous() and (x2 is None or x2.is_contiguous())
        if out is None:
            out = self._alloc(x1.shape[:-1] + (c1 + c2,), torch.uint8 if out_f8 else None)
        need = lib().fie_groupnorm_workspace_bytes(b, rows, groups)
        key = (self._stream, self.ws_tag)            # one scratch buffer per stream (and per in-flight graph slot)
        ws = self._scratch(self._gn_ws, key, need)
        if self._keep is not None:
            self._keep.append(ws)
        tag = getattr(x1, "_gn_tag", None)
        if (tag is not None and x2 is None and tag[1:5] == (groups, c1, rows, b) and tag[5] == self._gn_gen and tag[6] == key):
            # the producer's epilogue left this tensor's partial sums (and nothing has overwritten them): one read of x instead of two
            if out_f8:
                _chk(lib().fie_groupnorm_stats_nhwc_f16_o8(self.h, _p(x1), c1, _p(out), b, rows, groups, _p(gamma), _p(beta), float(eps), int(silu),
                                                           _p(tag[0]), _p(ws), tag[7], float(out_inv_scale)))
                return out
            _chk(lib().fie_groupnorm_stats_nhwc_f16(self.h, _p(x1), c1, _p(out), b, rows, groups, _p(gamma), _p(beta), float(eps), int(silu),
                                                    _p(tag[0]), _p(ws), tag[7]))
            return out
        if out_f8:
            _chk(lib().fie_groupnorm_nhwc_f16_o8(self.h, _p(x1), c1, _p(x2), c2, _p(out), b, rows, groups, _p(gamma), _p(beta), float(eps), int(silu), _p(ws),
                                                 float(out_inv_scale)))
            return out
        _chk((lib().fie_groupnorm_nhwc_f32 if self.f32 else lib().fie_groupnorm_nhwc_f16)(self.h, _p(x1), c1, _p(x2), c2, _p(out), b, rows, groups, _p(gamma),
                                          _p(beta), float(eps), int(silu), _p(ws)))
        return out

    def conv3x3_gn_ok(self, x, cout, out_groups):
        """True when GroupNorm(+SiLU) -> conv3x3 exists as ONE launch for this input (include/fie.h: fie_conv3x3_gn_ok) and x carries its producer's sums."""
        b, h, w, cin = x.shape
        return bool(self.gn_fuse_conv and not self.f32 and getattr(x, "_gn_tag", None) is not None and out_groups
                    and lib().fie_conv3x3_gn_ok(self.h, b, h, w, cin, cout, out_groups))

    def groupnorm_coef(self, x, gamma, beta, groups, eps):
        """The GroupNorm of x (which carries its producer's partial sums) as per-(image, channel) coefficients [B, C, 2] f32 (fie_groupnorm_coef_f16), or
        None when the sums are not there any more."""
        self.sync_stream()
        b, rows, c = x.shape[0], x[0].numel() // x.shape[-1], x.shape[-1]
        tag = getattr(x, "_gn_tag", None)
        key = (self._stream, self.ws_tag)
        if not (tag is not None and tag[1:5] == (groups, c, rows, b) and tag[5] == self._gn_gen and tag[6] == key):
            return None
        need = lib().fie_groupnorm_workspace_bytes(b, rows, groups)
        ws = self._scratch(self._gn_ws, key, need)
        if self._keep is not None:
            self._keep.append(ws)
        coef = self._alloc((b, c, 2), torch.float32)
        _chk(lib().fie_groupnorm_coef_f16(self.h, _p(x), c, b, rows, groups, _p(gamma), _p(beta), float(eps), _p(tag[0]), _p(ws), tag[7], _p(coef)))
        return coef

    def conv3x3_gn(self, x, coef, silu, wp, cout, bias=None, residual=None, gn_groups=None, out=None):
        """conv3x3(silu(x * sc + sh)) in one launch (fie_conv3x3_gn_nhwc_f16); the output's own GroupNorm sums are armed as for conv3x3."""
        self.sync_stream()
        self._bind_splitk()
        b, h, w, cin = x.shape
        assert x.is_contiguous() and coef.dtype == torch.float32 and coef.shape == (b, cin, 2)
        if out is None:
            out = self._alloc((b, h, w, cout))
        tag = self._gn_stats_arm(b * h * w, cout, h * w, gn_groups)
        assert tag is not None, "the fused GroupNorm -> conv needs the output's sums armed (conv3x3_gn_ok)"
        _chk(lib().fie_conv3x3_gn_nhwc_f16(self.h, _p(x), b, h, w, cin, _p(coef), int(bool(silu)), _p(wp), wp.stride(0), _p(out), out.stride(2), cout, _p(bias),
                                           _p(residual), residual.stride(2) if residual is not None else 0))
        out._gn_tag = tag
        return out

    def quantize_f8(self, x, inv_scale=1.0, out=None):
        """[rows, C] f16 -> e4m3 bytes (value * inv_scale, saturated): the plain conversion (tests; producers without a fused form)."""
        self.sync_stream()
        rows, c = x.shape
        if out is None:
            out = self._alloc((rows, c), torch.uint8)
        _chk(lib().fie_quantize_f8(self.h, _p(x), x.stride(0), _p(out), out.stride(0), rows, c, float(inv_scale)))
        return out

    def amax_into(self, x, slot):
        """Folds max |x| of a [..., C] f16 tensor (last dim contiguous, uniform row stride) into the device float `slot` (fp8 calibration)."""
        self.sync_stream()
        x2 = x.reshape(-1, x.shape[-1]) if x.is_contiguous() else x
        assert x2.dim() == 2 and x2.stride(1) == 1 and x2.dtype == torch.float16 and slot.dtype == torch.float32
        _chk(lib().fie_amax_f16(self.h, _p(x2), x2.stride(0), x2.shape[0], x2.shape[1], _p(slot)))

    def layernorm(self, x, gamma, beta, eps=1e-5, out=None, out_f8=False, out_inv_scale=1.0):
        self.sync_stream()
        rows, c = x.shape
        if out_f8:
            out = self._alloc((rows, c), torch.uint8) if out is None else out
            _chk(lib().fie_layernorm_f16_o8(self.h, _p(x), x.stride(0), _p(out), out.stride(0), rows, c, _p(gamma), _p(beta), float(eps), float(out_inv_scale)))
            return out
        if out is None:
            out = self._alloc((rows, c))
        _chk((lib().fie_layernorm_f32 if self.f32 else lib().fie_layernorm_f16)(self.h, _p(x), x.stride(0), _p(out), out.stride(0), rows, c, _p(gamma), _p(beta),
                                     float(eps)))
        return out

    def sinusoid(self, vals, dim, out, col0=0):
        """vals: f32 [B, nvals] on device; writes [cos|sin] blocks of width dim into out[:, col0:]."""
        self.sync_stream()
        b, nv = vals.shape
        _chk((lib().fie_sinusoid_f32 if self.f32 else lib().fie_sinusoid_f16)(self.h, _p(vals), b, nv, dim, _p(out), out.stride(0), col0))
        return out

    def time_embed_workspace(self, e):
        """Zero-filled workspace of the fused timestep-embedding kernel (one per model: launches on one stream reuse it)."""
        return torch.zeros(lib().fie_time_embed_workspace_bytes(e), device=self.device, dtype=torch.uint8)

    def time_embed(self, t, w1, b1, w2, b2, ws, add=None, out=None):
        """K7 fused: silu(W2 silu(W1 sinusoid(t) + b1) + b2 + add) for the B <= 4 rows of one step; w1 [E, C0], w2 [E, E] plain f16."""
        self.sync_stream()
        b, (e, c0) = t.numel(), w1.shape
        if out is None:
            out = self._alloc((b, e), torch.float16)
        _chk(lib().fie_time_embed_f16(self.h, _p(t), b, c0, e, _p(w1), _p(b1), _p(w2), _p(b2), _p(add),
                                      add.stride(0) if add is not None else 0, _p(out), out.stride(0), _p(ws)))
        return out

    def clip_embed(self, ids, tok, pos, out=None):
        self.sync_stream()
        b, t = ids.shape
        c = tok.shape[1]
        if out is None:
            out = self._alloc((b * t, c))
        assert out.is_contiguous()
        _chk((lib().fie_clip_embed_f32 if self.f32 else lib().fie_clip_embed_f16)(self.h, _p(ids), b, t, c, _p(tok), _p(pos), _p(out)))
        return out

    def pixels_in(self, u8_hwc, normalize, copies=1, out=None):
        self.sync_stream()
        h, w, _ = u8_hwc.shape
        if out is None:
            out = self._alloc((copies, h, w, 8))
        assert out.is_contiguous()
        _chk((lib().fie_pixels_in_u8_f32 if self.f32 else lib().fie_pixels_in_u8_f16)(self.h, _p(u8_hwc), h, w, int(normalize), _p(out), copies))
        return out

    def pixels_out(self, x_nhwc, out=None):
        self.sync_stream()
        _, h, w, ld = x_nhwc.shape
        if out is None:
            out = self._alloc((h, w, 3), torch.uint8)
        assert out.is_contiguous()
        _chk((lib().fie_pixels_out_f32_u8 if self.f32 else lib().fie_pixels_out_f16_u8)(self.h, _p(x_nhwc), ld, h, w, _p(out)))
        return out

    def resize_lanczos(self, rgb_u8, out_h, out_w, out=None):
        """u8 [H, W, 3] device tensor -> u8 [out_h, out_w, 3], bit-exact with PIL's `resize(..., Image.LANCZOS)`.  A u8 [H, W] tensor
        (a mode-L mask) -> u8 [out_h, out_w] through the one-band kernels (fie_resize_l_u8)."""
        self.sync_stream()
        assert rgb_u8.dtype == torch.uint8 and rgb_u8.is_contiguous()
        if rgb_u8.dim() == 2:
            return self._resize(rgb_u8, rgb_u8.shape[0], rgb_u8.shape[1], out_h, out_w, (), lib().fie_resize_l_u8, out=out)
        h, w, _ = rgb_u8.shape
        return self._resize(rgb_u8, h, w, out_h, out_w, (3,), lib().fie_resize_rgb_u8, out=out)

    def resize_bicubic(self, rgb_u8, out_h, out_w, out=None):
        """u8 [H, W, 3] device tensor -> u8 [out_h, out_w, 3], bit-exact with PIL's `resize(..., Image.BICUBIC)` (what CLIPImageProcessor resizes
        with): the kernels of resize_lanczos on BICUBIC tables.  `out`: a contiguous u8 [out_h, out_w, 3] tensor to write (a slice of a batch)."""
        self.sync_stream()
        assert rgb_u8.dtype == torch.uint8 and rgb_u8.is_contiguous() and rgb_u8.dim() == 3
        h, w, _ = rgb_u8.shape
        return self._resize(rgb_u8, h, w, out_h, out_w, (3,), lib().fie_resize_rgb_u8, filter="bicubic", out=out)

    def _resize(self, src, h, w, out_h, out_w, chan, entry, filter="lanczos", out=None):
        tabs = [self._axis_tables(w, out_w, filter), self._axis_tables(h, out_h, filter)]
        if out is None:
            out = torch.empty((out_h, out_w) + chan, device=src.device, dtype=torch.uint8)
        assert out.shape == (out_h, out_w) + chan and out.dtype == torch.uint8 and out.is_contiguous()
        tmp = torch.empty((h, out_w) + chan, device=src.device, dtype=torch.uint8) if (h != out_h and w != out_w) else None
        (kx, bx, ksx), (ky, by, ksy) = tabs
        _chk(entry(self.h, _p(src), h, w, _p(out), out_h, out_w, _p(kx), _p(bx), ksx, _p(ky), _p(by), ksy, _p(tmp)))
        return out

    def _feather_taps(self, blur):
        """The feather's Gaussian taps (fie_amd/mask.py: gaussian_taps) on the device, cached per sigma."""
        from . import mask as hmask
        cache = self.__dict__.setdefault("_mask_taps", {})
        key = float(blur)
        if key not in cache:
            cache[key] = torch.from_numpy(hmask.gaussian_taps(key)).to(self.device)
        return cache[key]

    def mask_prep(self, mask_l, blur=0.0, out=None):
        """Edit-size u8 [H, W] mask on the device (white = edit) -> (mask_px f32 [H, W], mask_lat u8 [H/8 * W/8]): one launch of
        fie_mask_prep.  mask_px is the binary mask L >= 128, or with blur = r > 0 its Gaussian feather (fie_amd/mask.py: gaussian_taps)."""
        self.sync_stream()
        h, w = mask_l.shape
        assert mask_l.dtype == torch.uint8 and mask_l.is_contiguous()
        taps = self._feather_taps(blur)
        if out is not None:                         # (mask_px, mask_lat) to write: contiguous tensors of the shapes below
            m_px, m_lat = out
            assert m_px.is_contiguous() and m_lat.is_contiguous()
        else:
            m_px = torch.empty((h, w), device=self.device, dtype=torch.float32)
            m_lat = torch.empty(((h // 8) * (w // 8),), device=self.device, dtype=torch.uint8)
        _chk(lib().fie_mask_prep(self.h, _p(mask_l), h, w, _p(taps), (taps.numel() - 1) // 2, _p(m_px), _p(m_lat)))
        return m_px, m_lat

    def mask_grow(self, mask_l, radius, out=None):
        """The mask grown (radius > 0) or shrunk (radius < 0) by the exact Euclidean disk of |radius| <= 64 pixels (fie_mask_grow_u8; DESIGN.md
        section 16).  mask_l: contiguous u8 [H, W] on the device (set = L >= 128), any size below 2^31 pixels.  -> u8 [H, W] of 0 / 255; radius 0
        the binarised mask.  `out`: a contiguous u8 [H, W] tensor to write (not the operand).  One launch, no synchronisation."""
        self.sync_stream()
        if not torch.is_tensor(mask_l) or mask_l.dim() != 2 or mask_l.dtype != torch.uint8 or not mask_l.is_contiguous():
            raise ValueError(f"mask_grow: a contiguous u8 [H, W] mask, got {tuple(getattr(mask_l, 'shape', ()))} {getattr(mask_l, 'dtype', type(mask_l).__name__)}")
        if isinstance(radius, bool) or not isinstance(radius, numbers.Integral):
            raise ValueError(f"mask_grow: radius={radius!r}: an integer")
        h, w = mask_l.shape
        if out is None:
            out = self._alloc((h, w), torch.uint8)
        elif tuple(out.shape) != (h, w) or out.dtype != torch.uint8 or not out.is_contiguous() or out.data_ptr() == mask_l.data_ptr():
            raise ValueError(f"mask_grow: out must be a contiguous u8 {(h, w)} tensor of its own")
        _chk(lib().fie_mask_grow_u8(self.h, _p(mask_l), h, w, int(radius), _p(out)))
        return out

    def mask_ramp(self, mask_l, radius, out=None):
        """A level map from a binary mask's outline (fie_mask_ramp_u8): 0 outside the mask (set = L >= 128), inside it
        floor(255 d / radius) clipped to 255, d the Euclidean distance to the nearest unset pixel of the image; radius in 1 .. 64.  mask_l:
        contiguous u8 [H, W] on the device, any size below 2^31 pixels.  -> u8 [H, W]; `out`: a contiguous u8 [H, W] tensor to write (not the
        operand).  One launch, no synchronisation."""
        self.sync_stream()
        if not torch.is_tensor(mask_l) or mask_l.dim() != 2 or mask_l.dtype != torch.uint8 or not mask_l.is_contiguous():
            raise ValueError(f"mask_ramp: a contiguous u8 [H, W] mask, got {tuple(getattr(mask_l, 'shape', ()))} {getattr(mask_l, 'dtype', type(mask_l).__name__)}")
        if isinstance(radius, bool) or not isinstance(radius, numbers.Integral):
            raise ValueError(f"mask_ramp: radius={radius!r}: an integer")
        h, w = mask_l.shape
        if out is None:
            out = self._alloc((h, w), torch.uint8)
        elif tuple(out.shape) != (h, w) or out.dtype != torch.uint8 or not out.is_contiguous() or out.data_ptr() == mask_l.data_ptr():
            raise ValueError(f"mask_ramp: out must be a contiguous u8 {(h, w)} tensor of its own")
        _chk(lib().fie_mask_ramp_u8(self.h, _p(mask_l), h, w, int(radius), _p(out)))
        return out

    def kv_emphasis(self, x, w, vflags):
        """Prompt emphasis on a text K | V result, in place (fie_kv_emphasis): x [rows, ncols] in the context's dtype with
        unit column stride and a row stride that is a multiple of 8; w f32 [rows] on the device, one weight per text row; vflags u8 [ncols / 8]
        on the device, non-zero over the V columns.  Flagged columns of every row with w != 1 are multiplied by its weight (one fp32 multiply,
        one rounding); rows of weight 1 and unflagged columns keep their bits.  One launch, no synchronisation.  -> x."""
        self.sync_stream()
        if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != self.dtype or x.stride(1) != 1:
            raise ValueError(f"kv_emphasis: a [rows, ncols] {self.dtype} tensor with unit column stride, got {tuple(getattr(x, 'shape', ()))} "
                             f"{getattr(x, 'dtype', type(x).__name__)}")
        rows, ncols = x.shape
        if not torch.is_tensor(w) or w.dtype != torch.float32 or w.dim() != 1 or w.numel() != rows or not w.is_contiguous():
            raise ValueError(f"kv_emphasis: w must be a contiguous f32 [{rows}] tensor, one weight per row")
        if not torch.is_tensor(vflags) or vflags.dtype != torch.uint8 or vflags.dim() != 1 or vflags.numel() * 8 != ncols or not vflags.is_contiguous():
            raise ValueError(f"kv_emphasis: vflags must be a contiguous u8 [{ncols // 8}] tensor, one flag per 8 columns of {ncols}")
        if w.device != x.device or vflags.device != x.device:
            raise ValueError("kv_emphasis: w and vflags live on the device of x")
        _chk(lib().fie_kv_emphasis(self.h, _p(x), x.stride(0), rows, ncols, _p(w), _p(vflags), int(self.f32)))
        return x

    def control_pyramid(self, e, a, binary, levels=3, out=None):
        """The control weights of one image (fie_control_pyramid_u8): e a contiguous u8 [H, W] tensor on the device, H, W
        multiples of 8 in 8 .. 2048 -- an L mask (binary=True: read as 255 where >= 128) or a level map (binary=False); a in 0 .. 255, the
        integer of `in_mask`.  -> f32 [P_tot], the weights of `levels` pyramid levels, finest first (fie_amd/control.py: weights_numpy);
        `out`: a contiguous f32 [P_tot] tensor to write.  One launch, no synchronisation."""
        from . import control
        self.sync_stream()
        if not torch.is_tensor(e) or e.dim() != 2 or e.dtype != torch.uint8 or not e.is_contiguous():
            raise ValueError(f"control_pyramid: a contiguous u8 [H, W] map, got {tuple(getattr(e, 'shape', ()))} {getattr(e, 'dtype', type(e).__name__)}")
        if isinstance(a, bool) or not isinstance(a, numbers.Integral) or not 0 <= a <= 255:
            raise ValueError(f"control_pyramid: a={a!r}: an integer in 0 .. 255")
        h, w = e.shape
        if h > 2048 or w > 2048:
            raise ValueError(f"control_pyramid: a map of {w}x{h} is above 2048")
        p_tot = sum(hl * wl for hl, wl in control.level_dims(h, w, levels))         # a ValueError for a size that is no multiple of 8
        if out is None:
            out = self._alloc((p_tot,), torch.float32)
        elif not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (p_tot,) or not out.is_contiguous() or out.device != e.device:
            raise ValueError(f"control_pyramid: out must be a contiguous f32 [{p_tot}] tensor on the device of e")
        _chk(lib().fie_control_pyramid_u8(self.h, _p(e), h, w, int(levels), int(a), int(bool(binary)), _p(out)))
        return out

    def control_add(self, segments, w, rows_per_image, outs=None):
        """out_i = u_i + (s_i * w[p]) * t_i for all residuals of one evaluation in one launch (fie_control_add).  segments:
        1 .. 16 tuples (u, t, P, woff, s) -- u, t contiguous tensors of one shape [..., C] in the context's dtype, C % 8 == 0, whose rows are B
        batch rows of P latent positions; woff: where the level of the residual starts in a row of w; s: its scale.  w: contiguous f32
        [images, P_tot] on the device; batch row b reads image b // rows_per_image.  -> the list of fresh output tensors, shaped like u.
        Where s * w is 0 the output is u's bits and t is not read.  `outs`: one contiguous tensor per segment to write, shaped like its u and
        no operand.  No synchronisation."""
        self.sync_stream()
        segments = list(segments)
        if outs is not None and len(outs) != len(segments):
            raise ValueError(f"control_add: {len(outs)} outs for {len(segments)} segments")
        n_max = header.DEFINES["CONTROL_MAX_SEGMENTS"]
        if not 1 <= len(segments) <= n_max:
            raise ValueError(f"control_add: {len(segments)} segments, 1 .. {n_max}")
        if not torch.is_tensor(w) or w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous() or w.device.type != self.device.type:
            raise ValueError("control_add: w must be a contiguous f32 [images, P_tot] tensor on the device")
        if isinstance(rows_per_image, bool) or not isinstance(rows_per_image, numbers.Integral) or rows_per_image < 1:
            raise ValueError(f"control_add: rows_per_image={rows_per_image!r}: a positive integer")
        images, p_tot = w.shape
        tab, made = ControlTable(), []
        tab.count = len(segments)
        for i, (u, t, p, woff, s) in enumerate(segments):
            ok = (torch.is_tensor(u) and torch.is_tensor(t) and u.dtype == self.dtype == t.dtype and u.dim() >= 2 and u.shape == t.shape
                  and u.is_contiguous() and t.is_contiguous() and u.device == w.device == t.device and u.numel() > 0)
            if not ok:
                raise ValueError(f"control_add: segment {i}: u and t are contiguous {self.dtype} tensors of one shape on the device of w")
            c, rows = u.shape[-1], u.numel() // u.shape[-1]
            if c % 8 or p < 1 or rows % p or woff < 0 or woff + p > p_tot:
                raise ValueError(f"control_add: segment {i}: C = {c} (C % 8 == 0), {rows} rows of P = {p} positions, weights {woff} .. {woff + p} of {p_tot}")
            if -(-(rows // p) // rows_per_image) > images:
                raise ValueError(f"control_add: segment {i}: {rows // p} batch rows at {rows_per_image} per image are more than the {images} images of w")
            if not isinstance(s, numbers.Real) or s != s:
                raise ValueError(f"control_add: segment {i}: s={s!r}: a number")
            if outs is None:
                out = self._alloc(tuple(u.shape))
            else:
                out = outs[i]
                if not (torch.is_tensor(out) and out.dtype == u.dtype and out.shape == u.shape and out.is_contiguous() and out.device == u.device
                        and out.data_ptr() not in (u.data_ptr(), t.data_ptr())):
                    raise ValueError(f"control_add: segment {i}: out must be a contiguous {self.dtype} tensor of u's shape, and a tensor of its own")
            made.append(out)
            tab.C[i], tab.P[i], tab.woff[i], tab.rows[i], tab.s[i] = c, p, woff, rows, float(s)
            tab.u[i], tab.t[i], tab.out[i] = _p(u), _p(t), _p(out)
        _chk(lib().fie_control_add(self.h, ctypes.byref(tab), _p(w), p_tot, int(rows_per_image), int(self.f32)))
        return made

    def mask_support(self, levels, out=None):
        """The support of a level map: u8 of any shape (contiguous) -> u8 of that shape, 255 where the level is > 0 (fie_mask_support_u8)."""
        self.sync_stream()
        if not torch.is_tensor(levels) or levels.dtype != torch.uint8 or not levels.is_contiguous() or levels.numel() == 0:
            raise ValueError("mask_support: a contiguous, non-empty u8 tensor")
        if out is None:
            out = self._alloc(tuple(levels.shape), torch.uint8)
        elif tuple(out.shape) != tuple(levels.shape) or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError(f"mask_support: out must be a contiguous u8 {tuple(levels.shape)} tensor")
        _chk(lib().fie_mask_support_u8(self.h, _p(levels), levels.numel(), _p(out)))
        return out

    def mask_levels(self, levels_e, mask_lat, out=None):
        """The latent levels of a soft mask (fie_mask_levels_u8): levels_e u8 [H, W] at the edit size, mask_lat u8 [H/8 * W/8] (mask_prep's, of
        the support) -> u8 [H/8 * W/8]: mask_lat ? max(levels_e[8y, 8x], 1) : 0."""
        self.sync_stream()
        if not torch.is_tensor(levels_e) or levels_e.dim() != 2 or levels_e.dtype != torch.uint8 or not levels_e.is_contiguous():
            raise ValueError("mask_levels: levels_e must be a contiguous u8 [H, W] tensor")
        h, w = levels_e.shape
        n = (h // 8) * (w // 8)
        if h % 8 or w % 8 or mask_lat.dtype != torch.uint8 or mask_lat.numel() != n or not mask_lat.is_contiguous():
            raise ValueError(f"mask_levels: H, W multiples of 8 and mask_lat a contiguous u8 tensor of {n} elements")
        if out is None:
            out = self._alloc((n,), torch.uint8)
        elif out.dtype != torch.uint8 or out.numel() != n or not out.is_contiguous():
            raise ValueError(f"mask_levels: out must be a contiguous u8 tensor of {n} elements")
        _chk(lib().fie_mask_levels_u8(self.h, _p(levels_e), _p(mask_lat), h, w, _p(out)))
        return out

    def outpaint_canvas(self, src, mask_l, margins, out=None):
        """The canvas of an outpainting edit and its mask (fie_outpaint_canvas_rgb_u8).  src: contiguous u8 [H, W, 3] on the
        device; mask_l: None or a contiguous u8 [H, W]; margins: (left, top, right, bottom), integers in 0 .. 4096, not all 0.  -> (canvas u8
        [Hc, Wc, 3], canvas_mask u8 [Hc, Wc]) with Hc = top + H + bottom, Wc = left + W + right: the source with its edge pixels replicated into
        the margins, and 255 in the margins over the mask as passed (0 without one).  `out`: a pair of contiguous u8 tensors of those shapes to
        write (neither an operand, nor each other).  One launch, no synchronisation."""
        self.sync_stream()
        if not torch.is_tensor(src) or src.dim() != 3 or src.shape[2] != 3 or src.dtype != torch.uint8 or not src.is_contiguous():
            raise ValueError(f"outpaint_canvas: a contiguous u8 [H, W, 3] source, got {tuple(getattr(src, 'shape', ()))} {getattr(src, 'dtype', type(src).__name__)}")
        h, w, _ = src.shape
        if mask_l is not None and (not torch.is_tensor(mask_l) or tuple(mask_l.shape) != (h, w) or mask_l.dtype != torch.uint8
                                   or not mask_l.is_contiguous()):
            raise ValueError(f"outpaint_canvas: mask_l must be None or a contiguous u8 {(h, w)} tensor, got "
                             f"{tuple(getattr(mask_l, 'shape', ()))} {getattr(mask_l, 'dtype', type(mask_l).__name__)}")
        try:
            margins = tuple(margins)
        except TypeError:
            margins = ()
        if len(margins) != 4 or any(isinstance(m, bool) or not isinstance(m, numbers.Integral) for m in margins):
            raise ValueError(f"outpaint_canvas: margins={margins!r}: four integers (left, top, right, bottom)")
        left, top, right, bottom = margins = tuple(int(m) for m in margins)
        if min(margins) < 0 or max(margins) > 4096 or not any(margins):
            raise ValueError(f"outpaint_canvas: margins={margins!r}: each in 0..4096 and at least one > 0")
        hc, wc = top + h + bottom, left + w + right
        if hc * wc >= 1 << 31:
            raise ValueError(f"outpaint_canvas: a canvas of {hc} x {wc} has 2^31 pixels or more")
        if out is None:
            out = self._alloc((hc, wc, 3), torch.uint8), self._alloc((hc, wc), torch.uint8)
        else:
            ops = [t.data_ptr() for t in (src, mask_l) if t is not None]
            ok = isinstance(out, (tuple, list)) and len(out) == 2 and all(torch.is_tensor(o) and o.dtype == torch.uint8 and o.is_contiguous() for o in out)
            if not ok or tuple(out[0].shape) != (hc, wc, 3) or tuple(out[1].shape) != (hc, wc) or out[0].data_ptr() in ops \
                    or out[1].data_ptr() in ops or out[0].data_ptr() == out[1].data_ptr():
                raise ValueError(f"outpaint_canvas: out must be a pair of contiguous u8 tensors {(hc, wc, 3)} and {(hc, wc)} of their own")
        _chk(lib().fie_outpaint_canvas_rgb_u8(self.h, _p(src), _p(mask_l), h, w, left, top, right, bottom, _p(out[0]), _p(out[1])))
        return out[0], out[1]

    def tile_blend(self, tiles, xs, ys, H, W, out=None):
        """The back end of a tiled edit (fie_tile_blend_rgb_u8).  tiles: contiguous u8 [ny * nx, th, tw, 3] on the device, tile
        j = iy * nx + ix at (xs[ix], ys[iy]); xs, ys: host lists of 1 .. 32 integers that start at 0, increase strictly, leave no gap and end at
        W - tw / H - th (anything else is a ValueError).  -> u8 [H, W, 3]: every pixel the weighted mean of the tiles that cover it, a tile's weight
        the distance to its nearest interior edge -- exactly fie_amd/tiles.py: blend_numpy.  `out`: a u8 [H, W, 3] tensor with contiguous
        memory at any address, not the tiles'.  One launch, no synchronisation."""
        from . import tiles as htiles
        self.sync_stream()
        if not torch.is_tensor(tiles) or tiles.dim() != 4 or tiles.shape[3] != 3 or tiles.dtype != torch.uint8 or not tiles.is_contiguous() \
                or tiles.numel() == 0:
            raise ValueError(f"tile_blend: contiguous u8 [n, th, tw, 3] tiles, got {tuple(getattr(tiles, 'shape', ()))} "
                             f"{getattr(tiles, 'dtype', type(tiles).__name__)}")
        n, th, tw, _ = tiles.shape
        if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1 for v in (H, W)) or H * W >= 1 << 31:
            raise ValueError(f"tile_blend: H={H!r}, W={W!r}: integers >= 1 with fewer than 2^31 pixels")
        H, W = int(H), int(W)
        xs, ys = htiles.check_positions(xs, tw, W, "xs"), htiles.check_positions(ys, th, H, "ys")
        if n != len(xs) * len(ys):
            raise ValueError(f"tile_blend: {n} tiles for a grid of {len(xs)} x {len(ys)}")
        if out is None:
            out = self._alloc((H, W, 3), torch.uint8)
        else:
            lo, hi = tiles.data_ptr(), tiles.data_ptr() + tiles.numel()
            if not torch.is_tensor(out) or tuple(out.shape) != (H, W, 3) or out.dtype != torch.uint8 or not out.is_contiguous() \
                    or (out.data_ptr() < hi and lo < out.data_ptr() + out.numel()):
                raise ValueError(f"tile_blend: out must be a contiguous u8 {(H, W, 3)} tensor of its own")
        cx, cy = (ctypes.c_int * len(xs))(*xs), (ctypes.c_int * len(ys))(*ys)
        _chk(lib().fie_tile_blend_rgb_u8(self.h, _p(tiles), len(xs), len(ys), cx, cy, th, tw, H, W, _p(out)))
        return out

    def mask_fill(self, src_u8, mask_l, ctl_u8=None, fill=True, out=None, cleared=None):
        """The masked-content pre-pass of a masked edit (fie_mask_fill_rgb_u8).  src_u8: u8 [H, W, 3]; mask_l: u8 [H, W]
        (hole = L >= 128); ctl_u8: None or the u8 [H, W, 3] edge map.  -> (filled, cleared): the source with the hole replaced by the push-pull
        continuation of its surroundings (None with fill=False: nothing is computed for it), and the edge map set to 0 inside the hole (None
        without ctl_u8).  No synchronisation; the pyramid's workspace is a fresh allocation of the caller's stream (a capture keeps it)."""
        self.sync_stream()
        h, w = mask_l.shape
        if mask_l.dtype != torch.uint8 or not mask_l.is_contiguous() or tuple(src_u8.shape) != (h, w, 3) or src_u8.dtype != torch.uint8 \
                or not src_u8.is_contiguous():
            raise ValueError(f"mask_fill: contiguous u8 [H, W, 3] image and u8 [H, W] mask, got {tuple(src_u8.shape)} {src_u8.dtype} and "
                             f"{tuple(mask_l.shape)} {mask_l.dtype}")
        if ctl_u8 is not None and (tuple(ctl_u8.shape) != (h, w, 3) or ctl_u8.dtype != torch.uint8 or not ctl_u8.is_contiguous()):
            raise ValueError(f"mask_fill: the edge map must be contiguous u8 {(h, w, 3)}, got {tuple(ctl_u8.shape)} {ctl_u8.dtype}")
        if not fill and ctl_u8 is None:
            raise ValueError("mask_fill: nothing to do (fill=False and no edge map)")
        ws = None
        if not fill:
            out = None
        if ctl_u8 is None:
            cleared = None
        if fill:
            nbytes = lib().fie_mask_fill_workspace_bytes(h, w)
            if nbytes < 0:
                raise FieError(f"mask_fill: {h} x {w} is outside 1 .. 2^24 pixels")
            ws = self._alloc((nbytes // 16, 4), torch.int32)
            if out is None:
                out = self._alloc((h, w, 3), torch.uint8)
        if ctl_u8 is not None and cleared is None:
            cleared = self._alloc((h, w, 3), torch.uint8)
        assert (out is None or out.is_contiguous()) and (cleared is None or cleared.is_contiguous())
        _chk(lib().fie_mask_fill_rgb_u8(self.h, _p(src_u8), _p(mask_l), h, w, _p(ws), _p(out), _p(ctl_u8), _p(cleared)))
        return out, cleared

    def multiband_workspace(self, h, w, levels):
        """The pyramid workspace of multiband_blend for an h x w image: a fresh int32 allocation of the caller's stream (a capture keeps it)."""
        nbytes = lib().fie_multiband_workspace_bytes(h, w, int(levels))
        if nbytes < 0:
            raise FieError(f"multiband_blend: {h} x {w} with {levels} levels is outside 1 .. 2^24 pixels, 1 .. 6 levels")
        return self._alloc((nbytes // 8, 2), torch.int32)

    def multiband_blend(self, edit_u8, source_u8, mask_l, alpha=None, levels=4, out=None, workspace=None):
        """The one-sided multi-band paste-back (fie_multiband_blend_rgb_u8).  edit_u8: u8 [H, W, 3], the decoded image;
        source_u8: u8 [H, W, 3], the resized source; mask_l: u8 [H, W] (edited = L >= 128).  -> u8 [H, W, 3]: the full blended image B, or with
        `alpha` (f32 [H, W], mask_prep's mask_px) its paste-back against the source.  `out`: a contiguous u8 [H, W, 3] tensor to write (no
        operand); `workspace`: multiband_workspace()'s, for a caller that keeps one.  No synchronisation, 2 * levels launches."""
        self.sync_stream()
        h, w = mask_l.shape
        u8img = lambda t: tuple(t.shape) == (h, w, 3) and t.dtype == torch.uint8 and t.is_contiguous()
        if mask_l.dtype != torch.uint8 or not mask_l.is_contiguous() or not u8img(edit_u8) or not u8img(source_u8):
            raise ValueError(f"multiband_blend: contiguous u8 [H, W, 3] images and a u8 [H, W] mask, got {tuple(edit_u8.shape)} {edit_u8.dtype}, "
                             f"{tuple(source_u8.shape)} {source_u8.dtype} and {tuple(mask_l.shape)} {mask_l.dtype}")
        if alpha is not None and (tuple(alpha.shape) != (h, w) or alpha.dtype != torch.float32 or not alpha.is_contiguous()):
            raise ValueError(f"multiband_blend: alpha must be contiguous f32 {(h, w)}, got {tuple(alpha.shape)} {alpha.dtype}")
        if out is None:
            out = self._alloc((h, w, 3), torch.uint8)
        elif not u8img(out) or any(out.data_ptr() == t.data_ptr() for t in (edit_u8, source_u8)):
            raise ValueError(f"multiband_blend: out must be a contiguous u8 {(h, w, 3)} tensor of its own")
        ws = workspace if workspace is not None else self.multiband_workspace(h, w, levels)
        need = lib().fie_multiband_workspace_bytes(h, w, int(levels))
        if need < 0 or ws.numel() * ws.element_size() < need:
            raise ValueError(f"multiband_blend: {h} x {w} with {levels} levels needs a workspace of {need} bytes")
        _chk(lib().fie_multiband_blend_rgb_u8(self.h, _p(edit_u8), _p(source_u8), _p(mask_l), _p(alpha), h, w, int(levels), _p(ws), _p(out)))
        return out

    def pixels_out_composite(self, x_nhwc, source_u8, mask_px, out=None):
        """pixels_out() with the paste-back: the source bytes where mask_px == 0, the decoded ones where it is 1, the rounded blend between."""
        self.sync_stream()
        _, h, w, ld = x_nhwc.shape
        assert source_u8.shape == (h, w, 3) and mask_px.shape == (h, w) and source_u8.is_contiguous() and mask_px.is_contiguous()
        if out is None:
            out = self._alloc((h, w, 3), torch.uint8)
        assert out.is_contiguous()
        _chk((lib().fie_pixels_out_composite_f32_u8 if self.f32 else lib().fie_pixels_out_composite_f16_u8)(
            self.h, _p(x_nhwc), ld, h, w, _p(source_u8), _p(mask_px), _p(out)))
        return out

    def _axis_tables(self, n_in, n_out, filter="lanczos"):
        """(taps, bounds, ksize) of one axis of the 8-bit resample on the device, cached per (in, out) size; (None, None, 0) when the axis keeps
        its size."""
        from . import resize
        if n_in == n_out:
            return None, None, 0
        key = (n_in, n_out) if filter == "lanczos" else (filter, n_in, n_out)
        if key not in self._resize_tables:
            kk, bounds, ks = resize.coefficients(n_in, n_out, filter)
            self._resize_tables[key] = (torch.from_numpy(kk).to(self.device), torch.from_numpy(bounds).to(self.device), ks)
        return self._resize_tables[key]

    def fullres_paste(self, res_u8, source_u8, mask_l=None, blur=0.0, out=None):
        """The full-resolution back end of an edit (fie_fullres_paste_rgb_u8).  res_u8: u8 [h, w, 3], the edit-size result;
        source_u8: u8 [H, W, 3], the source as uploaded; mask_l: None or u8 [H, W] (white = edit).  -> u8 [H, W, 3]: Pillow's LANCZOS resize of the
        result to (W, H), bit for bit, and with a mask the source byte where the mask's feather (sigma `blur`, in pixels of the H x W image) is 0, the
        resized byte where it is 1, the rounded blend between.  source_u8, mask_l and `out` may be views into larger images (unit strides inside a
        row, any row pitch, any byte offset); `out` may be source_u8.  Two launches on the current stream, no synchronisation."""
        self.sync_stream()
        h, w, _ = res_u8.shape
        H, W, _ = source_u8.shape
        rows_ok = lambda t: t.dtype == torch.uint8 and t.stride(-1) == 1 and (t.dim() == 2 or t.stride(1) == 3)
        if res_u8.dtype != torch.uint8 or not res_u8.is_contiguous() or res_u8.shape[2] != 3 or source_u8.shape[2] != 3 or not rows_ok(source_u8):
            raise ValueError("fullres_paste: res_u8 must be a contiguous u8 [h, w, 3] tensor, source_u8 a u8 [H, W, 3] tensor with contiguous rows")
        if out is None:
            out = torch.empty((H, W, 3), device=self.device, dtype=torch.uint8)
        if tuple(out.shape) != (H, W, 3) or not rows_ok(out):
            raise ValueError(f"fullres_paste: out must be a u8 {(H, W, 3)} tensor with contiguous rows")
        taps, radius = None, 0
        if mask_l is not None:
            if tuple(mask_l.shape) != (H, W) or not rows_ok(mask_l):
                raise ValueError(f"fullres_paste: mask_l must be a u8 {(H, W)} tensor with contiguous rows, got {tuple(mask_l.shape)} {mask_l.dtype}")
            taps = self._feather_taps(blur)
            radius = (taps.numel() - 1) // 2
        kx, bx, ksx = self._axis_tables(w, W)
        ky, by, ksy = self._axis_tables(h, H)
        tmp = torch.empty((h, W, 3), device=self.device, dtype=torch.uint8) if w != W else None
        _chk(lib().fie_fullres_paste_rgb_u8(self.h, _p(res_u8), h, w, _p(source_u8), source_u8.stride(0), _p(mask_l),
                                            mask_l.stride(0) if mask_l is not None else 0, H, W, _p(kx), _p(bx), ksx, _p(ky), _p(by), ksy,
                                            _p(taps), radius, _p(out), out.stride(0), _p(tmp)))
        return out

    def metrics_pairs(self, a, b, mask=None):
        """u8 [n, H, W, 3] (or [H, W, 3]) device tensors a, b -> int64 [n, 4] device tensor of fie_metrics_pairs_u8's result rows
        {sse, ssim_sum (float64 bits), bg_sse, bg_ssim_sum (float64 bits)}; fie_amd/metrics.py: rows_to_dicts decodes them on the host.
        `mask`: None, or u8 [n, H, W] (or [H, W]) with non-zero = edited region (the bg_* fields are 0 without one).  Two launches
        on the current stream, no synchronisation."""
        self.sync_stream()
        if a.dim() == 3:
            a, b, mask = a[None], b[None], None if mask is None else mask[None]
        n, h, w, c = a.shape
        if c != 3 or a.shape != b.shape or a.dtype != torch.uint8 or b.dtype != torch.uint8:
            raise ValueError(f"metrics_pairs: two u8 [n, H, W, 3] tensors of one shape, got {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype}")
        if mask is not None and (tuple(mask.shape) != (n, h, w) or mask.dtype != torch.uint8):
            raise ValueError(f"metrics_pairs: mask must be u8 {(n, h, w)}, got {tuple(mask.shape)} {mask.dtype}")
        a, b = a.contiguous(), b.contiguous()
        mask = None if mask is None else mask.contiguous()
        nbytes = lib().fie_metrics_workspace_bytes(n, h, w)
        if nbytes < 0:
            raise FieError(f"metrics_pairs: {h} x {w} images are below the 11 x 11 minimum of the SSIM window")
        ws = torch.empty(nbytes // 8, device=self.device, dtype=torch.int64)
        out = torch.empty((n, 4), device=self.device, dtype=torch.int64)
        _chk(lib().fie_metrics_pairs_u8(self.h, _p(a), _p(b), _p(mask), n, h, w, _p(out), _p(ws), nbytes))
        return out

    def sweep_select(self, imgs, rows, clip=None, rule="strongest", floor=float("-inf"), bg=False, out=None, out_idx=None):
        """The selector of a strength sweep (fie_sweep_select_u8).  imgs: 1 .. 16 u8 device tensors of one shape, each with
        contiguous memory at any address, strongest variant first; rows: the int64 [k, 4] device rows of metrics_pairs(); clip: None, or the f32
        [>= k, 2] device rows of clip_score() (rule "clip_score" needs them); floor: float64 in raw ssim_sum units (fie_amd/sweep.py: ssim_floor);
        bg: compare bg_ssim_sum.  -> (u8 tensor of the images' shape holding the winner, int32 [1] device tensor holding its index), exactly
        fie_amd/sweep.py: select_numpy.  `out` / `out_idx`: tensors to write into (out: the images' shape, contiguous memory at any address, not
        an image's).  One launch, no synchronisation."""
        from . import sweep as hsweep
        self.sync_stream()
        imgs = list(imgs)
        if not 1 <= len(imgs) <= hsweep.MAX_VARIANTS:
            raise ValueError(f"sweep_select: {len(imgs)} images: 1 .. {hsweep.MAX_VARIANTS}")
        if rule not in hsweep.RULES:
            raise ValueError(f"sweep_select: rule={rule!r}: one of {sorted(hsweep.RULES)}")
        k, shape = len(imgs), tuple(imgs[0].shape)
        for t in imgs:
            if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous() or t.numel() == 0:
                raise ValueError(f"sweep_select: contiguous u8 images of one shape, got {tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t).__name__)}")
        if not torch.is_tensor(rows) or rows.dtype != torch.int64 or tuple(rows.shape) != (k, 4) or not rows.is_contiguous():
            raise ValueError(f"sweep_select: rows must be a contiguous int64 {(k, 4)} tensor")
        if rule == "clip_score" and clip is None:
            raise ValueError("sweep_select: rule 'clip_score' needs the CLIP rows")
        if clip is not None and (not torch.is_tensor(clip) or clip.dtype != torch.float32 or clip.dim() != 2 or clip.shape[0] < k or clip.shape[1] != 2
                                 or not clip.is_contiguous()):
            raise ValueError(f"sweep_select: clip must be a contiguous f32 [>= {k}, 2] tensor")
        if out is None:
            out = self._alloc(shape, torch.uint8)
        elif not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"sweep_select: out must be a contiguous u8 {shape} tensor")
        if out_idx is None:
            out_idx = torch.empty(1, device=self.device, dtype=torch.int32)
        elif not torch.is_tensor(out_idx) or out_idx.dtype != torch.int32 or out_idx.numel() != 1:
            raise ValueError("sweep_select: out_idx must be an int32 tensor of one element")
        ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in imgs])
        _chk(lib().fie_sweep_select_u8(self.h, ptrs, k, imgs[0].numel(), _p(rows), _p(clip), hsweep.RULES[rule], float(floor), int(bool(bg)),
                                       _p(out), _p(out_idx)))
        return out, out_idx

    # ------------------------------------------------------------------ CLIP score (csrc/clip_score.hip)
    def clip_mask(self, rgb_u8, mask_l, out=None):
        """u8 [n, H, W, 3] (or [H, W, 3]) images with every pixel outside the edited region set to 0.  mask_l: u8 [n, MH, MW] (or [MH, MW]), L >= 128 =
        edited, of any size: sampled as Pillow's NEAREST resize to H x W would (fie_clip_mask_rgb_u8)."""
        from . import resize
        self.sync_stream()
        single = rgb_u8.dim() == 3
        a, m = (rgb_u8[None], mask_l[None]) if single else (rgb_u8, mask_l)
        n, h, w, c = a.shape
        if c != 3 or a.dtype != torch.uint8 or m.dtype != torch.uint8 or m.dim() != 3 or m.shape[0] != n or not a.is_contiguous() or not m.is_contiguous():
            raise ValueError(f"clip_mask: contiguous u8 [n, H, W, 3] images and u8 [n, MH, MW] masks, got {tuple(a.shape)} {a.dtype} and {tuple(m.shape)} {m.dtype}")
        mh, mw = m.shape[1:]
        tabs = []
        for n_in, n_out in ((mh, h), (mw, w)):
            key = ("nearest", n_in, n_out)
            if n_in != n_out and key not in self._resize_tables:
                self._resize_tables[key] = torch.from_numpy(resize.nearest_indices(n_in, n_out)).to(self.device)
            tabs.append(self._resize_tables.get(key) if n_in != n_out else None)
        if out is None:
            out = torch.empty_like(a)
        _chk(lib().fie_clip_mask_rgb_u8(self.h, _p(a), _p(m), n, h, w, mh, mw, _p(tabs[0]), _p(tabs[1]), _p(out)))
        return out[0] if single else out

    def clip_patches(self, rgb_u8, top, left, size, patch, mean, std):
        """u8 [n, H, W, 3] (the images after the processor's resize) -> [n * (size / patch)^2, 3 patch^2] in the context's dtype: centre crop at
        (top, left), /255, (x - mean) / std, patchify, cast -- one launch (fie_clip_patches_u8_*)."""
        self.sync_stream()
        n, h, w, c = rgb_u8.shape
        if c != 3 or rgb_u8.dtype != torch.uint8 or not rgb_u8.is_contiguous():
            raise ValueError(f"clip_patches: a contiguous u8 [n, H, W, 3] tensor, got {tuple(rgb_u8.shape)} {rgb_u8.dtype}")
        out = self._alloc((n * (size // max(patch, 1)) ** 2, 3 * patch * patch))
        fn = lib().fie_clip_patches_u8_f32 if self.f32 else lib().fie_clip_patches_u8_f16
        _chk(fn(self.h, _p(rgb_u8), n, h, w, int(top), int(left), int(size), int(patch), (_F * 3)(*mean), (_F * 3)(*std), _p(out)))
        return out

    def vit_embed(self, patches, cls, pos, n):
        """patches [n * P, C] (the patch GEMM's output), cls [C], pos [1 + P, C] -> the tower's input tokens [n * (1 + P), C] (fie_vit_embed_*)."""
        self.sync_stream()
        rows, c = patches.shape
        p = rows // n
        assert rows == n * p and pos.shape == (p + 1, c) and cls.numel() == c and patches.is_contiguous() and pos.is_contiguous() and cls.is_contiguous()
        out = self._alloc((n * (p + 1), c))
        _chk((lib().fie_vit_embed_f32 if self.f32 else lib().fie_vit_embed_f16)(self.h, _p(patches), _p(cls), _p(pos), n, p, c, _p(out)))
        return out

    def clip_score(self, img_emb, txt_emb, out=None):
        """[n, P] image and text embeddings (the context's dtype, last dim contiguous) -> f32 [n, 2] = (100 cos, max(100 cos, 0)) per pair, on the
        device (fie_clip_score_*): one launch, no synchronisation."""
        self.sync_stream()
        n, p = img_emb.shape
        if txt_emb.shape != img_emb.shape or img_emb.dtype != self.dtype or txt_emb.dtype != self.dtype or img_emb.stride(1) != 1 or txt_emb.stride(1) != 1:
            raise ValueError(f"clip_score: two [n, P] {self.dtype} tensors of one shape, got {tuple(img_emb.shape)} {img_emb.dtype} and {tuple(txt_emb.shape)} {txt_emb.dtype}")
        if out is None:
            out = self._alloc((n, 2), torch.float32)
        _chk((lib().fie_clip_score_f32 if self.f32 else lib().fie_clip_score_f16)(self.h, _p(img_emb), img_emb.stride(0), _p(txt_emb), txt_emb.stride(0), n, p, _p(out)))
        return out

    # ------------------------------------------------------------------ DINO structure distance (csrc/dino.hip)
    def _aa_tables(self, n_in, n_out):
        """Device tables of the antialias triangle filter (resize.py: aa_coefficients), cached per (in, out) size like the LANCZOS / BICUBIC ones."""
        from . import resize
        key = ("aa", n_in, n_out)
        if key not in self._resize_tables:
            ww, bounds, ks = resize.aa_coefficients(n_in, n_out)
            if (bounds[:, 0] < 0).any() or (bounds[:, 0] + bounds[:, 1] > n_in).any() or (bounds[:, 1] > ks).any():
                raise ValueError(f"aa_coefficients({n_in}, {n_out}): taps leave the input")
            self._resize_tables[key] = (torch.from_numpy(ww).to(self.device), torch.from_numpy(bounds).to(self.device), ks)
        return self._resize_tables[key]

    def dino_patches(self, rgb_u8, out_h, out_w, patch, mean, std, out=None):
        """u8 [n, H, W, 3] -> [n * (out_h / patch) * (out_w / patch), 3 patch^2] in the context's dtype: x / 255, torch's antialiased bilinear resize to
        out_h x out_w in fp32, (x - mean) / std, patchify, cast (fie_dino_patches_u8_*: two launches).  `out`: the rows of a larger patch matrix to write."""
        self.sync_stream()
        n, h, w, c = rgb_u8.shape
        if c != 3 or rgb_u8.dtype != torch.uint8 or not rgb_u8.is_contiguous():
            raise ValueError(f"dino_patches: a contiguous u8 [n, H, W, 3] tensor, got {tuple(rgb_u8.shape)} {rgb_u8.dtype}")
        rows, k = n * (out_h // max(patch, 1)) * (out_w // max(patch, 1)), 3 * patch * patch
        if out is None:
            out = self._alloc((rows, k))
        elif tuple(out.shape) != (rows, k) or out.dtype != self.dtype or not out.is_contiguous():
            raise ValueError(f"dino_patches: out must be a contiguous {self.dtype} {(rows, k)} tensor, got {tuple(out.shape)} {out.dtype}")
        wx, bx, ksx = self._aa_tables(w, out_w)
        wy, by, ksy = self._aa_tables(h, out_h)
        tmp = self._alloc((n, h, out_w, 3), torch.float32)
        fn = lib().fie_dino_patches_u8_f32 if self.f32 else lib().fie_dino_patches_u8_f16
        _chk(fn(self.h, _p(rgb_u8), n, h, w, int(out_h), int(out_w), _p(wx), _p(bx), ksx, _p(wy), _p(by), ksy, int(patch), (_F * 3)(*mean), (_F * 3)(*std),
                _p(tmp), _p(out)))
        return out

    def selfsim_mse(self, keys_a, keys_b, n, out=None):
        """keys_a, keys_b: [n * T, C] key matrices of n pairs (the context's dtype, last dim contiguous, one row stride: a column range of a fused qkv
        output) -> f64 [n] on the device: the mean over T x T of the squared difference of their cosine self-similarity matrices
        (fie_selfsim_mse_*: three launches, no synchronisation)."""
        self.sync_stream()
        rows, c = keys_a.shape
        t = rows // max(n, 1)
        if (n <= 0 or rows != n * t or keys_b.shape != keys_a.shape or keys_a.dtype != self.dtype or keys_b.dtype != self.dtype or keys_a.stride(1) != 1
                or keys_b.stride(1) != 1 or keys_a.stride(0) != keys_b.stride(0)):
            raise ValueError(f"selfsim_mse: two [n * T, C] {self.dtype} tensors of one shape and row stride, got {tuple(keys_a.shape)} {keys_a.dtype} and "
                             f"{tuple(keys_b.shape)} {keys_b.dtype} for n={n}")
        nbytes = lib().fie_selfsim_workspace_bytes(n, t)
        ws = self._alloc(((nbytes + 7) // 8,), torch.int64)
        if out is None:
            out = self._alloc((n,), torch.float64)
        _chk((lib().fie_selfsim_mse_f32 if self.f32 else lib().fie_selfsim_mse_f16)(self.h, _p(keys_a), _p(keys_b), keys_a.stride(0), n, t, c, _p(ws), _p(out)))
        return out

    # ------------------------------------------------------------------ LPIPS (csrc/lpips.hip): fp32 in every context
    def lpips_stem(self, rgb_u8, lut, w, bias, mask=None, out=None):
        """u8 [n, H, W, 3] (mask: None or u8 [n, H, W], non-zero = the pixel counts as black) -> f32 [n, OH, OW, 64]: the scaled input through
        the table `lut` f32 [3, 256], conv 3 -> 64 k3 stride 2 without padding (w f32 [27, 64], bias f32 [64]) and ReLU, one launch
        (fie_lpips_stem_u8_f32).  `out`: a contiguous f32 tensor of that shape to write (the images of a larger batch)."""
        self.sync_stream()
        n, h, wd, c = rgb_u8.shape
        if c != 3 or rgb_u8.dtype != torch.uint8 or not rgb_u8.is_contiguous() or h < 3 or wd < 3:
            raise ValueError(f"lpips_stem: a contiguous u8 [n, H, W, 3] tensor of at least 3 x 3, got {tuple(rgb_u8.shape)} {rgb_u8.dtype}")
        if mask is not None and (tuple(mask.shape) != (n, h, wd) or mask.dtype != torch.uint8 or not mask.is_contiguous()):
            raise ValueError(f"lpips_stem: mask must be a contiguous u8 {(n, h, wd)} tensor, got {tuple(mask.shape)} {mask.dtype}")
        f32c = lambda t, shape: t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()
        if not (f32c(lut, (3, 256)) and f32c(w, (27, 64)) and f32c(bias, (64,))):
            raise ValueError("lpips_stem: lut f32 [3, 256], w f32 [27, 64] and bias f32 [64], contiguous")
        shape = (n, (h - 3) // 2 + 1, (wd - 3) // 2 + 1, 64)
        if out is None:
            out = self._alloc(shape, torch.float32)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"lpips_stem: out must be a contiguous f32 {shape} tensor, got {tuple(out.shape)} {out.dtype}")
        _chk(lib().fie_lpips_stem_u8_f32(self.h, _p(rgb_u8), _p(mask), n, h, wd, _p(lut), _p(w), _p(bias), _p(out)))
        return out

    def maxpool3s2(self, x, out=None):
        """f32 [n, H, W, C] contiguous, C % 4 == 0 -> f32 [n, OH, OW, C]: MaxPool2d(3, stride 2, ceil_mode=True), bit-equal to torch's
        (fie_maxpool3s2_nhwc_f32; one launch)."""
        self.sync_stream()
        if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[3] % 4 or min(x.shape[1:3]) < 2:
            raise ValueError(f"maxpool3s2: a contiguous f32 [n, H, W, C] tensor of at least 2 x 2 with C % 4 == 0, got {tuple(x.shape)} {x.dtype}")
        n, h, w, c = x.shape
        shape = (n, (h - 2) // 2 + 1, (w - 2) // 2 + 1, c)
        if out is None:
            out = self._alloc(shape, torch.float32)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"maxpool3s2: out must be a contiguous f32 {shape} tensor, got {tuple(out.shape)} {out.dtype}")
        _chk(lib().fie_maxpool3s2_nhwc_f32(self.h, _p(x), n, h, w, c, _p(out)))
        return out

    def lpips_layer(self, fa, fb, w, out=None):
        """fa, fb: f32 [P, HW, C] contiguous, the same tap of the two sides of P pairs; w: f32 [C], the tap's `lin` weight -> f64 [P]: the mean
        over the pixels of sum_c w_c (fa / sqrt(1e-8 + |fa|^2) - fb / sqrt(1e-8 + |fb|^2))^2 (fie_lpips_layer_f32: two launches, no
        synchronisation).  `out`: a f64 [P] tensor or column of a [P, k] one to write."""
        self.sync_stream()
        ok = lambda t: t.dim() == 3 and t.dtype == torch.float32 and t.is_contiguous()
        if not ok(fa) or not ok(fb) or fa.shape != fb.shape or fa.shape[2] % 64 or fa.shape[2] > 512 or fa.shape[0] < 1 or fa.shape[1] < 1:
            raise ValueError(f"lpips_layer: two contiguous f32 [P, HW, C] tensors of one shape, C % 64 == 0 and C <= 512, got {tuple(fa.shape)} {fa.dtype} "
                             f"and {tuple(fb.shape)} {fb.dtype}")
        p, hw, c = fa.shape
        if w.dtype != torch.float32 or tuple(w.shape) != (c,) or not w.is_contiguous():
            raise ValueError(f"lpips_layer: w must be a contiguous f32 {(c,)} tensor, got {tuple(w.shape)} {w.dtype}")
        if out is None:
            out = self._alloc((p,), torch.float64)
        elif out.dtype != torch.float64 or tuple(out.shape) != (p,):
            raise ValueError(f"lpips_layer: out must be a f64 {(p,)} tensor, got {tuple(out.shape)} {out.dtype}")
        ws = self._alloc((lib().fie_lpips_layer_workspace_bytes(p, hw) // 8,), torch.int64)
        _chk(lib().fie_lpips_layer_f32(self.h, _p(fa), _p(fb), p, hw, c, _p(w), _p(ws), _p(out), out.stride(0)))
        return out

    def canny_device(self, rgb_u8, low=100, high=200, out=None, budget=None, workspace=None):
        """u8 [H, W, 3] device tensor -> u8 [H, W, 3] edge map on the device (integer exact; synchronises the stream).  `budget`: None, or the
        number of strong seeds an edge-budget Canny may keep (fie_amd/canny_auto.py: budget): the thresholds are picked on the device, (low, high)
        give their ratio, and `self.canny_pair` holds the pair that was used; `workspace`: as canny_begin()'s."""
        if budget is not None:
            edges, state = self.canny_begin(rgb_u8, low, high, rounds=1, budget=budget, out=out, workspace=workspace)
            return self.canny_finish(state)
        self.sync_stream()
        h, w, _ = rgb_u8.shape
        assert rgb_u8.is_contiguous() and rgb_u8.dtype == torch.uint8
        ws = torch.empty(lib().fie_canny_workspace_bytes(h, w), device=self.device, dtype=torch.uint8)
        if out is None:
            out = torch.empty((h, w, 3), device=self.device, dtype=torch.uint8)
        assert out.is_contiguous()
        it = _I(0)
        _chk(lib().fie_canny_rgb_device_u8(self.h, _p(rgb_u8), h, w, int(low), int(high), _p(ws), _p(out), ctypes.byref(it)))
        self.canny_passes = it.value
        return out

    def _canny_words(self):
        """The pinned words of the Canny on the current stream: 4 hysteresis flags, then the pair of an edge-budget Canny.  One set per stream
        (edits in flight run on their own)."""
        cache = self.__dict__.setdefault("_canny_flags", {})
        words = cache.get(self._stream)
        if words is None:
            words = cache[self._stream] = torch.zeros(6, dtype=torch.int32).pin_memory()
        return words

    def canny_begin(self, rgb_u8, low=100, high=200, rounds=1, budget=None, out=None, workspace=None):
        """First half of canny_device() (include/fie.h: fie_canny_rgb_device_begin_u8): launches NMS + `rounds` rounds of four hysteresis passes + the
        edge map and returns (edge map tensor, state) without waiting; canny_finish(state) waits and tells whether that map was final.
        `budget`: as canny_device()'s (fie_canny_rgb_device_begin_auto_u8: ridge + histogram, select and classify kernels in place of the NMS
        kernel; still no wait).  `workspace`: a u8 tensor of fie_canny_auto_workspace_bytes to use (edge-budget form only)."""
        self.sync_stream()
        h, w, _ = rgb_u8.shape
        assert rgb_u8.is_contiguous() and rgb_u8.dtype == torch.uint8
        if out is None:
            out = torch.empty((h, w, 3), device=self.device, dtype=torch.uint8)
        assert out.is_contiguous()
        flags = self._canny_words()
        if budget is None:
            ws = torch.empty(lib().fie_canny_workspace_bytes(h, w), device=self.device, dtype=torch.uint8)
            _chk(lib().fie_canny_rgb_device_begin_u8(self.h, _p(rgb_u8), h, w, int(low), int(high), int(rounds), _p(ws), _p(out), flags.data_ptr()))
        else:
            ws = self._canny_auto_workspace(h, w, workspace)
            _chk(lib().fie_canny_rgb_device_begin_auto_u8(self.h, _p(rgb_u8), h, w, int(budget), int(low), int(high), int(rounds), _p(ws), _p(out),
                                                          flags.data_ptr()))
        return out, (h, w, ws, out, flags, rgb_u8, int(rounds), budget is not None)

    def _canny_auto_workspace(self, h, w, workspace=None):
        need = lib().fie_canny_auto_workspace_bytes(h, w)
        if need < 0:
            raise ValueError(f"edge-budget Canny: no workspace for an image of {h} x {w}")
        if workspace is None:
            return torch.empty(need, device=self.device, dtype=torch.uint8)
        assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.numel() >= need
        return workspace

    def canny_finish(self, state):
        """Waits for canny_begin's work; runs the further hysteresis rounds if its last pass had still changed something (the edge map tensor is then
        rewritten).  Returns the tensor; `self.canny_more` = passes launched here (0: the map was final when begin's kernels ended).  After an
        edge-budget begin, `self.canny_pair` = the (low, high) the device used, read from the pinned words."""
        h, w, ws, out, flags, _src, rounds, auto = state
        self.sync_stream()
        it = _I(0)
        _chk(lib().fie_canny_rgb_device_finish_u8(self.h, h, w, _p(ws), _p(out), flags.data_ptr(), ctypes.byref(it)))
        self.canny_more = it.value
        self.canny_passes = 4 * rounds + it.value
        if auto:
            self.canny_pair = (int(flags[4]), int(flags[5]))
        return out

    def canny_thresholds(self, rgb_u8, budget, lo=100, hi=200, workspace=None):
        """The (low, high) an edge-budget Canny of the u8 [H, W, 3] device tensor uses under `budget` and the ratio lo / hi, as Python ints
        (fie_canny_thresholds_device_u8: ridge + histogram and select; SYNCHRONISES: the 8 bytes are read back)."""
        self.sync_stream()
        h, w, _ = rgb_u8.shape
        assert rgb_u8.is_contiguous() and rgb_u8.dtype == torch.uint8
        ws = self._canny_auto_workspace(h, w, workspace)
        pair = torch.empty(2, device=self.device, dtype=torch.int32)
        _chk(lib().fie_canny_thresholds_device_u8(self.h, _p(rgb_u8), h, w, int(budget), int(lo), int(hi), _p(ws), _p(pair)))
        low, high = pair.cpu().tolist()
        return low, high

    def _latent_prep(self, entry, moments, eps_post, noise, hw, sf, sqrt_ab, sqrt_1mab, latents, model_in, *tail):
        """The fie_latent_prep* entry `entry` (its _f32 twin in an fp32 context): the arguments all three share, then the entry's own."""
        self.sync_stream()
        _chk(getattr(lib(), entry + ("_f32" if self.f32 else ""))(
            self.h, _p(moments), _p(eps_post), _p(noise), hw, float(sf), float(sqrt_ab), float(sqrt_1mab), _p(latents), _p(model_in),
            model_in.shape[0], *tail))

    def latent_prep(self, moments, eps_post, noise, hw, sf, sqrt_ab, sqrt_1mab, latents, model_in):
        self._latent_prep("fie_latent_prep", moments, eps_post, noise, hw, sf, sqrt_ab, sqrt_1mab, latents, model_in)

    def latent_prep_src(self, moments, eps_post, noise, hw, sf, sqrt_ab, sqrt_1mab, latents, model_in, z0):
        """latent_prep() that also stores the clean source latent z0 (f32 [hw, 4]) for a masked edit."""
        self._latent_prep("fie_latent_prep_src", moments, eps_post, noise, hw, sf, sqrt_ab, sqrt_1mab, latents, model_in, _p(z0))

    def latent_prep_src_content(self, moments, eps_post, noise, hw, sf, sqrt_ab, sqrt_1mab, latents, model_in, z0, mask_lat, mode):
        """latent_prep_src() with a masked-content mode (fie_amd/mask.py: CONTENT_MODES names them): where mask_lat != 0 the initial latent is
        the init noise itself ("latent_noise") or sqrt_1mab * noise ("latent_nothing"); everything else keeps latent_prep_src's bits."""
        from . import mask as hmask
        self._latent_prep("fie_latent_prep_src_content", moments, eps_post, noise, hw, sf, sqrt_ab, sqrt_1mab, latents, model_in, _p(z0),
                          _p(mask_lat), hmask.CONTENT_CODES[mode])

    def _lcm_step(self, entry, eps, nb, guidance, latents, noise, hw, sab_t, s1mab_t, c_skip, c_out, sab_p, s1mab_p, model_in, inv_sf, decode_in,
                  *tail):
        """The fie_lcm_step* entry `entry` (its _f32 twin in an fp32 context): the arguments all three share, then the entry's own."""
        self.sync_stream()
        _chk(getattr(lib(), entry + ("_f32" if self.f32 else ""))(
            self.h, _p(eps), eps.shape[-1], nb, float(guidance), _p(latents), _p(noise), hw, float(sab_t), float(s1mab_t), float(c_skip),
            float(c_out), float(sab_p), float(s1mab_p), _p(model_in), model_in.shape[0] if model_in is not None else 0, float(inv_sf),
            _p(decode_in), *tail))

    def lcm_step(self, eps, nb, guidance, latents, noise, hw, sab_t, s1mab_t, c_skip, c_out, sab_p, s1mab_p, model_in,
                 inv_sf, decode_in):
        self._lcm_step("fie_lcm_step", eps, nb, guidance, latents, noise, hw, sab_t, s1mab_t, c_skip, c_out, sab_p, s1mab_p, model_in,
                       inv_sf, decode_in)

    def lcm_step_masked(self, eps, nb, guidance, latents, noise, hw, sab_t, s1mab_t, c_skip, c_out, sab_p, s1mab_p, model_in,
                        inv_sf, decode_in, mask_lat, z0, noise_init):
        """lcm_step() followed, in the same pass, by the blend of a masked edit: latent pixels with mask_lat == 0 take
        sab_p z0 + s1mab_p noise_init (z0 on the last step, noise None)."""
        self._lcm_step("fie_lcm_step_masked", eps, nb, guidance, latents, noise, hw, sab_t, s1mab_t, c_skip, c_out, sab_p, s1mab_p, model_in,
                       inv_sf, decode_in, _p(mask_lat), _p(z0), _p(noise_init))

    def lcm_step_levels(self, eps, nb, guidance, latents, noise, hw, sab_t, s1mab_t, c_skip, c_out, sab_p, s1mab_p, model_in,
                        inv_sf, decode_in, lvl_lat, z0, noise_init, steps, step):
        """lcm_step_masked() of a soft mask: lvl_lat u8 [hw] holds levels 0 .. 255, `step` is this step's place among
        the `steps` of the edit; a latent pixel of level v is inside iff v * steps > 255 * (steps - 1 - step)."""
        self._lcm_step("fie_lcm_step_levels", eps, nb, guidance, latents, noise, hw, sab_t, s1mab_t, c_skip, c_out, sab_p, s1mab_p, model_in,
                       inv_sf, decode_in, _p(lvl_lat), _p(z0), _p(noise_init), int(steps), int(step))


def canny_rgb(rgb_u8, low=100, high=200):
    """Host Canny through the C ABI (numpy uint8 HxWx3 in and out)."""
    import numpy as np
    a = np.ascontiguousarray(rgb_u8, dtype=np.uint8)
    out = np.empty_like(a)
    _chk(lib().fie_canny_rgb_u8(a.ctypes.data, a.shape[0], a.shape[1], int(low), int(high), out.ctypes.data))
    return out


def canny_auto_thresholds(rgb_u8, budget, lo=100, hi=200):
    """The (low, high) of an edge-budget Canny through the host C ABI entry (numpy uint8 HxWx3 in, two Python ints out; no device)."""
    import numpy as np
    a = np.ascontiguousarray(rgb_u8, dtype=np.uint8)
    pair = (ctypes.c_int * 2)()
    _chk(lib().fie_canny_auto_thresholds_u8(a.ctypes.data, a.shape[0], a.shape[1], int(budget), int(lo), int(hi), pair))
    return pair[0], pair[1]


_ctx = {}


def context(device=0, dtype=torch.float16):
    key = (device, dtype)
    if key not in _ctx:
        _ctx[key] = Context(device, dtype)
    return _ctx[key]
