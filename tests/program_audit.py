"""Audit of recorded launch programs (engine.Program): buffer lifetimes, pointer extents, reads of memory nothing wrote.

A helper, not collected (tests/test_program_audit_gpu.py drives it).  A launch program is a list of C-ABI calls whose arguments are
raw device pointers; its scratch comes from a free list keyed by the exact element count and goes back to it by hand.  Nothing in
that layer can be seen from eps or an image at a fixture shape, so this module looks at the RECORDED program instead:

  Recorder     patches Program.alloc / Program.release (on the class: NetBuilder, unet_small and autoencoder are covered without
               touching them) so that nothing is recycled and every buffer's allocation and release are on record.
  audit()      the static rules, evaluated without launching anything -- they hold for every shape the builder code can take:
                 R1 use after release        R2 release hygiene (the recorder's own report)      R3 persistent buffers
                 R4 dangling pointers        R5 extents (include/ldmk.h against the buffers the builders hand in)
  drive() / poison()   the dynamic rules' tools: run a program the way forward() does, on a workspace the test owns.

Every comparison is a set membership or an integer inequality; no tolerance appears here."""
import ast
import bisect
import collections
import ctypes as C
import gc
import os
import sys

import torch

from dsml_thesis_amd import engine, lib as L

PKG = os.path.dirname(os.path.abspath(engine.__file__))
PRODUCT_FILES = ("engine.py", "unet.py", "unet_small.py", "autoencoder.py")

Finding = collections.namedtuple("Finding", "rule message")


class Buffer:
    """One Program.alloc (or, program None, a scratch the engine made itself: split-K slabs, arrival counters, GroupNorm scratch)."""

    def __init__(self, program, tensor, shape, calls_at, site):
        self.program, self.tensor, self.shape, self.dtype = program, tensor, tuple(int(s) for s in shape), tensor.dtype
        self.base, self.nbytes = tensor.data_ptr(), tensor.numel() * tensor.element_size()
        self.alloc_at, self.alloc_site = calls_at, site
        self.released_at = self.release_site = None

    @property
    def end(self):
        return self.base + self.nbytes

    def __repr__(self):
        s = f"{list(self.shape)} {str(self.dtype).replace('torch.', '')} allocated at {self.alloc_site}"
        return s + (f", released at {self.release_site}" if self.release_site else "")


def _in_engine(frame, names):
    return (os.path.basename(frame.f_code.co_filename) == "engine.py" and os.path.dirname(os.path.abspath(frame.f_code.co_filename)) == PKG
            and frame.f_code.co_name in names)


def _where(frame):
    f = os.path.abspath(frame.f_code.co_filename)
    return f"{os.path.basename(f) if os.path.dirname(f) == PKG else f}:{frame.f_lineno}"


class Recorder:
    """Context manager: while active no Program recycles a buffer, and every alloc / release is on record.

    buffers        every Program.alloc, in order (Buffer)
    hygiene        rule R2 findings, reported rather than raised so that one run lists everything
    release_lines  (product file, line) of every frame of a product file that was on the stack of a Program.release: a `.release(`
                   call site is executed exactly when its line is among them (release_call_sites() lists the sites)"""

    def __init__(self):
        self.buffers, self.hygiene, self.release_lines, self.builders = [], [], set(), []
        self._sorted = []          # (base, index into buffers)

    # ---- lookup
    def _add(self, b):
        self.buffers.append(b)
        bisect.insort(self._sorted, (b.base, len(self.buffers) - 1))

    def find(self, ptr):
        """the buffer whose byte range contains ptr (interior pointers are normal), or None"""
        i = bisect.bisect_right(self._sorted, (ptr, len(self.buffers))) - 1
        if i >= 0:
            b = self.buffers[self._sorted[i][1]]
            if b.base <= ptr < b.end:
                return b
        return None

    def adopt(self, pg):
        """the scratch the engine allocates itself (Program.splitk_workspace / splitk_counters / post): in `_all`, never pooled"""
        for t in pg._all:
            if t.numel() and self.find(t.data_ptr()) is None:
                self._add(Buffer(None, t, t.shape, 0, "engine (shared scratch)"))

    # ---- the patches
    def __enter__(self):
        rec = self
        self._saved = (engine.Program.alloc, engine.Program.release, engine.NetBuilder.__init__)
        nb_init = engine.NetBuilder.__init__

        def alloc(pg, *shape, dtype=torch.float32):
            n = 1
            for s in shape:
                n *= int(s)
            t = torch.empty(n, device=pg.device, dtype=dtype)          # never recycled
            pg._all.append(t)
            f = sys._getframe(1)
            while f is not None and _in_engine(f, ("alloc_ps", "stats_buffer")):
                f = f.f_back
            if n:
                rec._add(Buffer(pg, t, shape, len(pg.calls), _where(f)))
            return t.view(*shape)

        def release(pg, *tensors):
            f = caller = sys._getframe(1)
            direct = not _in_engine(caller, ("release", "drop_stats"))
            while f is not None and _in_engine(f, ("release", "drop_stats")):
                f = f.f_back
            site = _where(f)
            g = caller
            while g is not None:
                path = os.path.abspath(g.f_code.co_filename)
                if os.path.dirname(path) == PKG and os.path.basename(path) in PRODUCT_FILES:
                    rec.release_lines.add((os.path.basename(path), g.f_lineno))
                g = g.f_back
            for t in tensors:
                if t is None:
                    continue
                b = rec.find(t.data_ptr()) if t.numel() else None
                if b is None or b.program is not pg:
                    rec.hygiene.append(Finding("R2", f"foreign release at {site}: a tensor {list(t.shape)} that did not come from this "
                                                     f"program's alloc" + (f" (it is {b!r})" if b is not None else "")))
                    continue
                if t.data_ptr() != b.base or t.numel() * t.element_size() != b.nbytes:
                    rec.hygiene.append(Finding("R2", f"partial-view release at {site}: {list(t.shape)} at byte {t.data_ptr() - b.base} of {b!r}"))
                    continue
                if b.released_at is not None:
                    rec.hygiene.append(Finding("R2", f"double release at {site} of {b!r}"))
                    continue
                b.released_at, b.release_site = len(pg.calls), site          # (NOT returned to the pool)
                if direct:
                    for nb in rec.builders:
                        if nb.pg is pg and t.data_ptr() in nb._stats:
                            rec.hygiene.append(Finding("R2", f"stale GroupNorm statistics: direct Program.release at {site} of {b!r} while "
                                                             "NetBuilder._stats still holds a record under its address"))

        def init(nb, *a, **kw):
            nb_init(nb, *a, **kw)
            rec.builders.append(nb)

        engine.Program.alloc, engine.Program.release, engine.NetBuilder.__init__ = alloc, release, init
        return self

    def __exit__(self, *exc):
        engine.Program.alloc, engine.Program.release, engine.NetBuilder.__init__ = self._saved
        return False


def release_call_sites():
    """every `<something>.release(...)` call of the four product files: [(file, first line, last line, the call's source text)]"""
    sites = []
    for name in PRODUCT_FILES:
        with open(os.path.join(PKG, name)) as f:
            src = f.read()
        for node in ast.walk(ast.parse(src)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "release":
                sites.append((name, node.lineno, node.end_lineno, ast.get_source_segment(src, node)))
    return sorted(sites)


def executed(site, release_lines):
    name, lo, hi = site[:3]
    return any(f == name and lo <= ln <= hi for f, ln in release_lines)


# ------------------------------------------------------------------------------------------------------------ pointer extraction
def _struct_of(call):
    _, _, keep, name = call
    return keep if name == "ldmk_igemm" else keep[0] if name == "ldmk_post" else None


def pointers(call):
    """(label, address) of every device pointer a recorded call carries: the c_void_p positions of lib._SIGS (the trailing stream
    is not part of a recorded call) and, for the two struct entry points, every c_void_p field of the struct in the keepalive slot"""
    _, args, _, name = call
    argtypes = L._SIGS[name][1][:-1]
    assert len(argtypes) == len(args), (name, len(argtypes), len(args))
    for i, (ty, v) in enumerate(zip(argtypes, args)):
        if ty is C.c_void_p:
            yield f"arg{i}", int(v or 0)
    st = _struct_of(call)
    if st is not None:
        for fname, fty in st._fields_:
            if fty is C.c_void_p:
                yield fname, int(getattr(st, fname) or 0)


# ------------------------------------------------------------------------------------------------------------ R5: extents
F32 = 4
_ATTN_KV = {  # flat attention entry points: (n, tokens, heads) start at this argument; the size query of kv_scratch (argument 1)
    "ldmk_attn_self_x3p": (3, "ldmk_attn_kv_split_bytes", None), "ldmk_attn_self_x3p_ps": (4, "ldmk_attn_kv_split_bytes", "ldmk_ps_bytes"),
    "ldmk_attn_self_h2": (4, "ldmk_attn_kv_split_h2_bytes", None), "ldmk_attn_self_h2_ps": (5, "ldmk_attn_kv_split_h2_bytes", "ldmk_ps_bytes_h2"),
    "ldmk_attn_self_h2_tiles": (5, "ldmk_attn_kv_split_h2_bytes", "ldmk_ps_bytes_h2"),
}


def igemm_extents(lib, a):
    """bytes an ldmk_igemm call may touch behind each pointer field, from include/ldmk.h -> ([(field, bytes)], [messages])"""
    ext, bad = [], []
    B = max(1, a.batch)
    ncol = a.N // 2 if a.epi == L.EPI_GEGLU else a.N
    raw = bool(a.raw_slabs) and a.splitk > 1             # `out`, `bias`, `batch_vec`, `residual` and `epi` are then not used
    psb = lib.ldmk_ps_bytes_h2 if a.compute == L.COMPUTE_F16X2 else lib.ldmk_ps_bytes
    samples = -(-a.M // max(1, a.rows_per_sample))

    def ps(field, rows, k, lead=0):
        nb = psb(int(rows), int(k))
        if nb <= 0:
            bad.append(f"{field}: no PS layout for a [{rows}][{k}] matrix")
        else:
            ext.append((field, lead + nb))

    if not raw:
        tile = ((B - 1) * a.out_bstride + (a.M - 1) * a.ldc + ncol) * F32
        ext += [("out", tile), ("residual", tile), ("bias", a.N * F32),
                ("batch_vec", ((samples - 1) * a.batch_vec_ld + a.N) * F32)]
    if a.a_tf in (L.TF_AFFINE, L.TF_AFFINE_SILU):
        ext.append(("tf_coef", samples * 2 * (a.c0 + a.c1) * F32))
    if a.a_tf in (L.TF_LAYERNORM, L.TF_LAYERNORM_FOLDED):
        ext.append(("row_stats", a.M * 2 * F32))
    if a.a_tf == L.TF_LAYERNORM:
        ext += [("ln_gamma", a.K * F32), ("ln_beta", a.K * F32)]
    if a.a_tf == L.TF_LAYERNORM_FOLDED:
        ext.append(("ln_colsum", a.N * F32))
    conv = a.a_mode == L.A_CONV3X3
    pixels = (a.M // max(1, a.out_h * a.out_w)) * a.in_h * a.in_w if conv else a.M       # stored rows of the A tensors
    if not a.a_ps:
        lead = (B - 1) * a.a_bstride
        ext += [("a0", (lead + pixels * a.c0) * F32), ("a1", (lead + pixels * a.c1) * F32)]
    ext += [("skip_a0", a.M * a.skip_c0 * F32), ("skip_a1", a.M * a.skip_c1 * F32)]
    if a.b_trans:
        ext.append(("w", ((B - 1) * a.w_bstride + (a.N - 1) * a.ldb + a.K) * F32))
    else:
        ext.append(("w", ((B - 1) * a.w_bstride + (a.K - 1) * a.ldb + a.N) * F32))
    ext.append(("stats_out", (a.M // 32) * a.N * 3 * F32))
    ext.append(("range_flag", 4))
    if a.a_split:
        ext.append(("a_split", 3 * a.M * a.a_split_ld * 2))
    # split-K scratch: the capacity the call states must lie inside the buffer AND cover what the pinned plan needs
    need = lib.ldmk_igemm_workspace_elems(C.byref(a))
    if need < 0:
        bad.append(f"ldmk_igemm_workspace_elems refuses the recorded arguments ({need})")
    elif need > a.splitk_ws_elems or (need > 0 and not a.splitk_ws):
        bad.append(f"splitk_ws: the plan (tile_cfg {a.tile_cfg}, splitk {a.splitk}) needs {need} floats, the call offers {a.splitk_ws_elems}")
    ext.append(("splitk_ws", a.splitk_ws_elems * F32))
    if a.splitk_counters:
        tiles = -(-a.M // 64) * -(-a.N // 64) * B
        if a.splitk_counters_len < tiles:
            bad.append(f"splitk_counters: {a.splitk_counters_len} counters for {tiles} output tiles")
        ext.append(("splitk_counters", a.splitk_counters_len * 4))
    if a.a_ps:
        lead = (B - 1) * a.a_ps_bstride
        if conv:
            ps("a_ps", pixels, a.c0 + a.c1, lead)
        elif a.a_ps1:
            ps("a_ps", a.M, a.a_ps_k0, lead)
            ps("a_ps1", a.M, a.K - a.a_ps_k0)
        else:
            ps("a_ps", a.M, a.K, lead)
        ps("w_ps", a.N, a.K, (B - 1) * a.w_ps_bstride)
    if a.out_ps:
        ps("out_ps", a.M, a.ldc)
    if a.attn_kv_out:
        if a.attn_tokens <= 0 or a.M % a.attn_tokens:
            bad.append(f"attn_kv_out: attn_tokens {a.attn_tokens} does not divide M {a.M}")
        else:
            ext.append(("attn_kv_out", lib.ldmk_attn_kv_split_h2_bytes(a.M // a.attn_tokens, a.attn_tokens, a.attn_heads)))
    return ext, bad


def post_extents(lib, a):
    ext, bad = [], []
    samples = -(-a.M // max(1, a.rows_per_sample))
    ncol = a.N // 2 if a.geglu else a.N
    ext += [("src", ((a.nslab - 1) * a.slab_stride + a.M * a.N) * F32), ("bias", a.N * F32),
            ("batch_vec", ((samples - 1) * a.batch_vec_ld + a.N) * F32), ("residual", ((a.M - 1) * a.ldr + a.N) * F32),
            ("raw_out", ((a.M - 1) * a.ld_raw + ncol) * F32), ("x1", a.M * a.c1 * F32)]
    if a.norm != L.POST_NONE:
        ext += [("gamma", (a.N + a.c1) * F32), ("beta", (a.N + a.c1) * F32), ("norm_out", ((a.M - 1) * a.ld_norm + a.N + a.c1) * F32)]
    need = lib.ldmk_post_scratch_elems(C.byref(a))
    if need < 0 or need > a.gn_scratch_elems or (need > 0 and not a.gn_scratch):
        bad.append(f"gn_scratch: ldmk_post_scratch_elems = {need}, the call offers {a.gn_scratch_elems}")
    ext.append(("gn_scratch", a.gn_scratch_elems * F32))
    return ext, bad


def flat_extents(lib, call):
    _, args, _, name = call
    hit = _ATTN_KV.get(name)
    if hit is None:
        return [], []
    at, kv_bytes, ps_bytes = hit
    n, tokens, heads = (int(v) for v in args[at:at + 3])
    ext = [("arg0", n * tokens * 3 * heads * 32 * F32), ("arg1", getattr(lib, kv_bytes)(n, tokens, heads)), ("arg2", n * tokens * heads * 32 * F32)]
    if ps_bytes is not None:
        ext.append(("arg3", getattr(lib, ps_bytes)(n * tokens, heads * 32)))
    return ext, []


# ------------------------------------------------------------------------------------------------------------ the static audit
def active_blocks():
    """[(address, end)] of the blocks of torch's caching allocator that a live tensor owns, sorted"""
    out = []
    for seg in torch.cuda.memory_snapshot():
        addr = seg["address"]
        for blk in seg["blocks"]:
            addr = blk.get("address", addr)          # (older snapshots carry no block address: the running sum of the sizes)
            if blk["state"] == "active_allocated":
                out.append((addr, addr + blk["size"]))
            addr += blk["size"]
    return sorted(out)


def _block_of(blocks, ptr):
    i = bisect.bisect_right(blocks, (ptr, 1 << 62)) - 1
    if i >= 0 and blocks[i][0] <= ptr < blocks[i][1]:
        return blocks[i]
    return None


class Report:
    def __init__(self):
        self.findings, self.pointers, self.calls = [], 0, 0

    def rules(self):
        return sorted({f.rule for f in self.findings})

    def __str__(self):
        return f"{self.calls} calls, {self.pointers} pointer arguments, {len(self.findings)} findings" + "".join(
            f"\n  {f.rule}: {f.message}" for f in self.findings)


def audit(rec, pg, snapshot=True):
    """R1-R5 on the program `pg` (and its ctx_program) as recorded under `rec`.  Call it after the builder has returned and
    outside the recorder; nothing is launched.

    R4's limit: a pointer passes when it lies in ANY block a live tensor owns.  A temporary whose block the allocator has
    already handed to another live tensor therefore passes; what R4 catches is the pointer whose block is still free when the
    build is over (which is what the next allocation -- the caller's input, a sampler's state -- then lands on).

    R5 measures a pointer outside the pool (weights, flags) against the end of its allocator block, which is the tensor's size
    rounded up (512 bytes and more): exact for every pool buffer, lenient by that rounding for the model's own tensors."""
    rep = Report()
    rep.findings += rec.hygiene                                   # R2
    lib = L.load()
    ctx = getattr(pg, "ctx_program", None)
    programs = [pg] + ([ctx] if ctx is not None else [])
    for p in programs:
        rec.adopt(p)
    blocks = None
    if snapshot:
        gc.collect()
        blocks = active_blocks()

    # R3: inputs, outputs and everything the context program touches stay allocated (the context program runs once per context
    # while the main program runs every step: a recycled buffer of it would be overwritten between two steps)
    for kind, d in (("input", getattr(pg, "inputs", {})), ("output", getattr(pg, "outputs", {}))):
        for k, t in d.items():
            b = None if t is None else rec.find(t.data_ptr())
            if b is not None and b.released_at is not None:
                rep.findings.append(Finding("R3", f"the program's {kind} '{k}' was released: {b!r}"))
    if ctx is not None:
        seen = set()
        for i, call in enumerate(ctx.calls):
            for label, ptr in pointers(call):
                b = rec.find(ptr) if ptr else None
                if b is not None and b.released_at is not None and id(b) not in seen:
                    seen.add(id(b))
                    rep.findings.append(Finding("R3", f"ctx_program call {i} {call[3]}.{label} uses a buffer that was released: {b!r}"))

    for p in programs:
        for i, call in enumerate(p.calls):
            name = call[3]
            rep.calls += 1
            where = {}
            for label, ptr in pointers(call):
                if not ptr:
                    continue
                rep.pointers += 1
                b = rec.find(ptr)
                if b is not None:
                    where[label] = (ptr, b.end, repr(b))
                    # R1: a call recorded at or after the release holds the pointer (a buffer of the other program has no common
                    # call index: any release of it is one)
                    if b.released_at is not None and (b.program is not p or b.released_at <= i):
                        rep.findings.append(Finding("R1", f"call {i} {name}.{label} reads or writes {b!r} after its release "
                                                          f"(released before call {b.released_at} of its program)"))
                elif blocks is not None:
                    blk = _block_of(blocks, ptr)
                    if blk is None:
                        rep.findings.append(Finding("R4", f"call {i} {name}.{label} = {ptr:#x} lies in no pool buffer and in no block "
                                                          "that a live tensor owns (a build-time temporary that nothing keeps alive)"))
                    else:
                        where[label] = (ptr, blk[1], f"a live torch block of {blk[1] - blk[0]} bytes")
            # R5
            st = _struct_of(call)
            if name == "ldmk_igemm":
                ext, bad = igemm_extents(lib, st)
            elif name == "ldmk_post":
                ext, bad = post_extents(lib, st)
            else:
                ext, bad = flat_extents(lib, call)
            rep.findings += [Finding("R5", f"call {i} {name}: {m}") for m in bad]
            for label, nbytes in ext:
                if label in where and nbytes > 0:
                    ptr, end, what = where[label]
                    if ptr + nbytes > end:
                        rep.findings.append(Finding("R5", f"call {i} {name}.{label}: the call may touch {nbytes} bytes, {end - ptr} remain in {what}"))
    return rep


# ------------------------------------------------------------------------------------------------------------ dynamic rules
def drive(pg, inputs):
    """What forward() does, directly: inputs in, context program, program, outputs out."""
    for k, v in inputs.items():
        dst = pg.inputs[k]
        dst.copy_(v.to(device=dst.device, dtype=dst.dtype).reshape(dst.shape))
    ctx = getattr(pg, "ctx_program", None)
    if ctx is not None:
        ctx.run()
    pg.run()
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in pg.outputs.items()}


def workspace(pg):
    """every tensor of the program's (and its context program's) workspace, once"""
    ctx = getattr(pg, "ctx_program", None)
    seen, out = set(), []
    for t in pg._all + ([] if ctx is None or ctx._all is pg._all else ctx._all):
        if id(t) not in seen:
            seen.add(id(t))
            out.append(t)
    return out


def poison(pg):
    """0xFF into every byte of the workspace: NaN in fp32 / fp16 / bf16, -1 in the integer types.  Exempt, and nothing else:
    the arrival counters of the in-launch split-K combine, which engine.Program.splitk_counters creates with torch.zeros and
    every GEMM launch leaves zeroed (`self._skcnt = torch.zeros(n, ...)`) -- of the program and of its context program."""
    ctx = getattr(pg, "ctx_program", None)
    exempt = {id(t) for t in (pg._skcnt, None if ctx is None else ctx._skcnt) if t is not None}
    for t in workspace(pg):
        if id(t) not in exempt and t.numel():
            t.view(torch.uint8).fill_(255)
    torch.cuda.synchronize()


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def finite(out):
    return all(bool(torch.isfinite(v).all()) for v in out.values() if v.dtype.is_floating_point)
