"""The C-ABI library loads and exports every symbol include/gfla_hip.h declares; host-side
argument checks behave like the reference's (no compute is launched here)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    """Expand the GFLA_DECL_* macros of the header by hand: every `gfla_<name>_##SFX` under a
    macro that is instantiated with (sfx, type)."""
    text = open(os.path.join(ROOT, "include", "gfla_hip.h")).read()
    names = set(re.findall(r"^(?:int|int64_t|const char \*)\s*(gfla_\w+)\(", text, flags=re.M))
    for macro, body in re.findall(r"#define (GFLA_DECL_\w+)\(SFX, T\)(.*?)\n(?=GFLA_DECL)", text, flags=re.S):
        bases = re.findall(r"(gfla_\w+?)_##SFX", body)
        for sfx in re.findall(macro + r"\((\w+), \w+\)", text):
            if sfx == "SFX":
                continue
            names.update("%s_%s" % (b, sfx) for b in bases)
    return names


def test_header_and_library_agree(gfla):
    from global_flow_local_attention_amd import _lib
    gfla.build()
    declared = _declared_symbols()
    assert declared == set(gfla.exported_symbols()), declared ^ set(gfla.exported_symbols())
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(handle, name), name
    assert _lib.lib().gfla_abi_version() == _lib.ABI_VERSION == 8


def test_argument_types_match_header(gfla):
    """The binding's types are derived from the header (_lib.parse_header).  The expectations below are written by hand from
    reading include/gfla_hip.h; the properties after them hold for every exported symbol."""
    from global_flow_local_attention_amd import _lib
    P, L, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    expected = {
        "gfla_fc_tail_fwd_f32": [P, L, L, P, P, P, P, P, L, L, L, I, D, P],
        "gfla_fc_tail_bwd_f64": [P, L, L, P, P, P, P, P, P, P, P, L, L, L, I, D, P],
        "gfla_convert_multi": [P, P, L, P, P, L, P, P, L, P, P, L, I, P],
        "gfla_gemm_f64": [P, P, P, P, P, P, L, L, L, I, I, P, P],
        "gfla_flow_warp_fwd_f16": [P, P, P, L, L, L, L, L, L, D, D, D, D, P],
        "gfla_instance_norm_bwd_bf16": [P, P, P, P, P, P, P, P, P, P, L, L, L, L, D, I, P],
        "gfla_head_conv3x3_bwd_f16": [P, P, P, P, P, P, P, P, P, P, L, L, L, L, L, L, I, I, D, I, I, P],
        "gfla_fc_backward_f32": [P, P, P, P, P, P, P, P, P, P, P, P, L, L, L, L, I, D, I, I, P],
        "gfla_big_plane_geometry": [I, L, L, L, L, L, L, I, I, P],
        "gfla_resample2d_bwd_ws_f32": [P, P, P, P, P, P, L, L, L, L, L, L, I, I, I, P],
        "gfla_block_extractor_unfold_bwd_f16": [P, P, P, P, P, L, L, L, L, L, L, I, I, P],   # GFLA_DECL_BWD16
        "gfla_maxpool2x2_bwd_bf16": [P, P, P, L, L, L, L, P],                                # GFLA_DECL_MAXPOOL2X2
        "gfla_abi_version": [],
        "gfla_status_string": [I],
        "gfla_xcd_swizzle": [L, L],
    }
    handle = _lib.lib()
    for name, args in expected.items():
        assert list(getattr(handle, name).argtypes) == args, name
    # which declarations end in a stream, and which return int64_t: read straight from the header's text (each macro body
    # with the suffixes it is instantiated with), not from the parser under test
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gfla_hip.h")).read(), flags=re.S).replace("\\\n", " ")
    with_stream, pointer_last, returns_i64 = set(), set(), set()
    scopes = [(("",), "\n".join(line for line in text.splitlines() if not line.startswith("#")))]      # plain declarations
    for macro, body in re.findall(r"^#define (GFLA_DECL_\w+)\(SFX, T\)(.*)$", text, flags=re.M):        # and each macro's
        scopes.append(([sfx for sfx in re.findall(macro + r"\((\w+), \w+\)", text) if sfx != "SFX"], body))
    for suffixes, scope in scopes:
        for ret, name, args in re.findall(r"\b(int64_t|int|const char \*)\s*(gfla_[\w#]+)\(([^)]*)\)\s*;", scope):
            names = [name.replace("##SFX", sfx) for sfx in suffixes]
            if re.search(r"gfla_stream_t stream\s*$", args):
                with_stream.update(names)
            elif "*" in args.split(",")[-1]:   # gfla_*_geometry's `int64_t *out`, gfla_fc_wino_debug_buffer's `void *buffer`
                pointer_last.update(names)
            if ret == "int64_t":
                returns_i64.update(names)
    symbols = gfla.exported_symbols()
    assert len(symbols) == len(set(symbols)) == 154 and (with_stream | pointer_last | returns_i64) <= set(symbols)
    assert len(with_stream) == 130 and len(returns_i64) == 12          # counted by hand in the header
    assert pointer_last == {"gfla_big_plane_geometry", "gfla_aggregate_fwd_geometry", "gfla_fc_geometry", "gfla_fc_wino_debug_buffer",
                            "gfla_instance_norm_geometry", "gfla_head_conv3x3_geometry"}
    for name in symbols:
        fn = getattr(handle, name)
        assert fn.argtypes is not None, name
        last_is_pointer = len(fn.argtypes) > 0 and fn.argtypes[-1] is P
        assert last_is_pointer == (name in with_stream or name in pointer_last), name
        assert (fn.restype is L) == (name in returns_i64), name
        assert fn.restype in (I, L) or name == "gfla_status_string", name
    assert handle.gfla_status_string.restype is ctypes.c_char_p
    # constants come from the header as well
    assert (_lib.PATH_BE_BWD_LDS, _lib.PATH_FC_BWD_MODE0, _lib.PATH_GEMM_F64, _lib.PATH_COUNT) == (0, 7, 20, 22)
    assert _lib.fc_path(3) == 5 and _lib.fc_path(2, backward=True) == 9 and _lib.fc_path(5) == 18


def test_header_parser_is_strict():
    from global_flow_local_attention_amd import _lib
    fns, consts = _lib.parse_header("enum e { A = 1, B = -2 };\n#define N 7\nint64_t gfla_f(const float *x, int n, gfla_stream_t stream);")
    assert fns == {"gfla_f": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])}
    assert consts == {"A": 1, "B": -2, "N": 7}
    for decl in ("int gfla_f(float x, int n)",           # float by value: no such argument in this ABI
                 "int gfla_f(int64_t n, size_t m)",
                 "int gfla_f(n)",
                 "float gfla_f(int n)",                  # unknown return types
                 "void *gfla_f(int n)",
                 "struct gfla_s { int a; }"):            # neither a declaration, a typedef nor an enum
        with pytest.raises(ValueError) as info:
            _lib.parse_header("int gfla_ok(int n);\n%s;\n" % decl)
        assert decl.split(";")[0] in str(info.value), (decl, str(info.value))


def test_workspace_helper(gfla, monkeypatch):
    """_lib.workspace on a stub library: a refusal of the size query is an exception that names the op, never a size handed
    to torch.empty, and the buffer is never empty (an empty tensor's pointer is NULL)."""
    import types
    from global_flow_local_attention_amd import _lib
    asked = []

    def query(answer):
        def fn(*sizes):
            asked.append(sizes)
            return answer
        return fn
    stub = types.SimpleNamespace(gfla_status_string=_lib.lib().gfla_status_string, q_unsupported=query(-3), q_shape=query(-2),
                                 q_null=query(-1), q_zero=query(0), q_some=query(1000))
    monkeypatch.setattr(_lib, "_lib", stub)
    ref = torch.zeros(1)
    with pytest.raises(_lib.Unsupported, match="some op"):
        _lib.workspace("q_unsupported", ref, 1, 2, what="some op")
    for name in ("q_shape", "q_null"):
        with pytest.raises(ValueError, match="some op") as info:
            _lib.workspace(name, ref, 1, 2, what="some op")
        assert not isinstance(info.value, _lib.Unsupported)
        assert _lib.lib().gfla_status_string(-2 if name == "q_shape" else -1).decode() in str(info.value)
    buf = _lib.workspace("q_zero", ref, 3, what="some op")
    assert buf.dtype == torch.uint8 and buf.numel() == 16 and buf.device == ref.device
    assert _lib.workspace("q_some", ref, 4.0, True, what="x").numel() == 1000
    assert asked[-1] == (4, 1) and all(type(v) is int for v in asked[-1])             # sizes cross as ints


def test_argument_validation_without_gpu(gfla):
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    n = None
    assert L.gfla_block_extractor_fwd_f32(n, n, n, 1, 1, 4, 4, 4, 4, 3, n) == -1  # NULL pointer
    assert L.gfla_local_attn_reshape_fwd_f32(n, n, 1, 4, 4, 3, n) == -1
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.gfla_block_extractor_fwd_f32(p, p, p, 0, 1, 4, 4, 4, 4, 3, n) == -2   # bad shape
    assert L.gfla_resample2d_fwd_f32(p, p, p, 1, 1, 4, 4, 4, 4, 1, 1, n) == -2     # kernel_size < 2
    assert L.gfla_local_attn_aggregate_fwd_f32(p, p, p, p, n, 1, 1, 4, 4, 4, 4, 9, 1, n) == -3  # k > 5
    assert b"NULL" in L.gfla_status_string(-1)


def test_cpu_tensors_are_rejected_like_the_reference(gfla):
    # block_extractor.py:23-24 / local_attn_reshape.py:20-21 raise NotImplementedError on CPU
    with pytest.raises(NotImplementedError):
        gfla.BlockExtractor(3)(torch.zeros(1, 1, 4, 4), torch.zeros(1, 2, 4, 4))
    with pytest.raises(NotImplementedError):
        gfla.LocalAttnReshape()(torch.zeros(1, 9, 4, 4), 3)
    with pytest.raises(NotImplementedError):
        gfla.Resample2d(4, 1, 2)(torch.zeros(1, 1, 4, 4), torch.zeros(1, 2, 4, 4))
    with pytest.raises(NotImplementedError):
        gfla.ExtractorAttn(4, 3, softmax=True)(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(1, 2, 4, 4))


def test_module_surface_matches_reference(gfla):
    m = gfla.ExtractorAttn(16, 5, torch.nn.LeakyReLU(0.1), softmax=True)
    assert list(m.state_dict().keys()) == ["fully_connect_layer.0.weight", "fully_connect_layer.0.bias",
                                           "fully_connect_layer.2.weight", "fully_connect_layer.2.bias"]
    assert m.fully_connect_layer[0].weight.shape == (128, 32, 5, 5)
    assert m.fully_connect_layer[2].weight.shape == (25, 128, 1, 1)
    assert isinstance(m.fully_connect_layer[3], torch.nn.Softmax)
    assert isinstance(gfla.ExtractorAttn(16, 4).fully_connect_layer[3], torch.nn.LeakyReLU)  # softmax=None
    assert gfla.BlockExtractor().kernel_size == 3
    r = gfla.Resample2d()
    assert (r.kernel_size, r.dilation) == (2, 1)
    assert len(list(r.parameters())) == 0 and len(list(r.buffers())) == 0


@pytest.mark.skipif(not os.path.isdir("/root/reference/model/networks"), reason="reference checkout not present")
def test_install_into_unmodified_reference(gfla):
    import subprocess, sys
    code = r"""
import sys, types
sys.path.insert(0, %r)
import global_flow_local_attention_amd as g
sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
bf = g.install('/root/reference')
import model.networks.generator as gen
net = gen.PoseGenerator(image_nc=3, structure_nc=18, ngf=64, img_f=512, layers=3, num_blocks=2, use_spect=False,
                        attn_layer=[2, 3], norm='instance', activation='LeakyReLU', extractor_kz={'2': 5, '3': 3})
assert type(net.target.attn0.extractor) is g.BlockExtractor
assert type(net.target.attn0.reshape) is g.LocalAttnReshape
assert bf.ExtractorAttn.forward.__module__ == 'global_flow_local_attention_amd.extractor_attn'
assert abs(sum(p.numel() for p in net.parameters()) - 14047395) == 0
print('ok')
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_aggregate_forward_table_path_geometry_invariants():
    """Host-side launch logic of the coefficient-table aggregation forward (csrc/local_attn_aggregate.hip), swept over
    shapes without a GPU: whatever it picks has to fit the hardware (160 KB of LDS, 12 waves per workgroup), cover every
    channel and tile, keep the staging within its per-thread budget of word pairs, and keep the LDS pitch on the
    conflict-free residue; the scratch the size query promises has to hold a record for every tile slot."""
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int64 * 9)()
    seen = 0
    for B in (1, 2, 8, 32, 256):
        for C in (1, 3, 16, 64, 128, 256, 512):
            for (H, W) in ((8, 8), (32, 22), (64, 44), (64, 64), (32, 32), (128, 88), (256, 176), (7, 6), (9, 130)):
                for k in (1, 3, 5):
                    rc = L.gfla_aggregate_fwd_geometry(B, C, H, W, H, W, k, ctypes.cast(out, ctypes.c_void_p))
                    if W < k + 1 or W % 2:
                        assert rc == -3
                        continue
                    if rc == -3:      # plane too large for two LDS buffers: the plain kernels take it
                        assert H * W * 4 * 2 > 60 * 1024
                        continue
                    assert rc == 0, (B, C, H, W, k, rc)
                    CH, CS, ns, tg, threads, pitch, tw, ntile, lds = list(out)
                    seen += 1
                    assert 1 <= CH <= C and CS % CH == 0 and ns * CS >= C and (ns - 1) * CS < C
                    assert threads % 64 == 0 and 64 <= threads <= 12 * 64
                    assert tw in (8, 16, 32) and ntile == -(-W // tw) * -(-H // (64 // tw))
                    assert tg * (threads // 64) >= ntile                    # every tile has a wave
                    assert pitch >= 2 * W and pitch % 64 == 32
                    per_plane = -(-H // 2) * pitch * 4
                    assert lds == 2 * (CH * per_plane + 16) and lds <= 160 * 1024
                    assert CH * H * (W // 2) <= 8 * threads                 # word pairs per thread and chunk
                    assert L.gfla_aggregate_fwd_workspace_bytes(B, H, W, k) >= B * ntile * 64 * (((k + 1) * (k + 2) + 4) // 4 * 4) * 4
    assert seen > 300


def test_host_helpers_of_the_launch_merges(gfla):
    """Round 4's host-side helpers, on CPU tensors: the one-allocation zero arena of the attention backward (segments on
    256-byte boundaries, the requested shapes, None for gradients nobody wants) and convert_many's pass-through rules
    (anything but a bf16 <-> f32 CUDA conversion goes to torch; None stays None; nothing to convert = the same tensors)."""
    import torch
    from global_flow_local_attention_amd import _lib, extractor_attn
    a, b, c = extractor_attn._zeros_f32(torch.device("cpu"), ((2, 3, 5, 7), True), ((2, 2, 5, 7), False), ((2, 9, 5, 7), True))
    assert b is None and a.shape == (2, 3, 5, 7) and c.shape == (2, 9, 5, 7)
    assert a.dtype == c.dtype == torch.float32 and not a.any() and not c.any()
    assert a.is_contiguous() and c.is_contiguous()
    assert a.untyped_storage().data_ptr() == c.untyped_storage().data_ptr()          # one allocation ...
    assert (c.data_ptr() - a.data_ptr()) % 256 == 0 and c.data_ptr() - a.data_ptr() >= a.numel() * 4   # ... aligned segments
    a.fill_(1.0)
    assert not c.any()
    x32, x16 = torch.randn(5, 3), torch.randn(4).to(torch.bfloat16)
    out = _lib.convert_many([x32, None, x16], torch.float32)
    assert out[0] is x32 or torch.equal(out[0], x32)
    assert out[1] is None and out[2].dtype == torch.float32 and torch.equal(out[2], x16.float())
    back = _lib.convert_many([x32], torch.bfloat16)
    assert back[0].dtype == torch.bfloat16 and torch.equal(back[0], x32.to(torch.bfloat16))


def test_big_plane_tile_geometry_and_xcd_remap_invariants(gfla):
    """Host logic of round 5's tile kernels (csrc/tile_map.h) without a GPU.  Geometry: whatever it picks must fit the
    hardware (<= 512 threads in whole waves, one pixel per thread, LDS request within the budget and at least 16 KB), cover
    the map with its tiles and the channels with its groups, start tiles on 32-column boundaries, and leave at least three
    workgroups per CU when the problem has them.  Regime: BASELINE configs[1] is in, the bench shapes (planes in LDS) and
    many-plane problems are out.  Remap: a bijection of [0, nwg) for any nwg, and the blocks of one XCD (block % 8) get one
    contiguous range."""
    from global_flow_local_attention_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int64 * 10)()
    po = ctypes.cast(out, ctypes.c_void_p)
    seen = 0
    for op in (0, 1, 2, 3, 4):
        for B in (1, 2, 32):
            for C in (1, 3, 64, 256):
                for (H, W) in ((256, 176), (7, 5), (64, 44), (33, 600), (1, 1), (500, 31)):
                    for span in (3, 4, 6, 9):
                        assert L.gfla_big_plane_geometry(op, B, C, H, W, H, W, span, 4, po) == 0
                        regime, th, tw, ntx, nty, threads, G, ngroups, lds, nwg = list(out)
                        seen += 1
                        assert threads % 64 == 0 and th * tw <= threads <= 512 and th >= 1 and tw >= 1
                        assert ntx * tw >= W and (ntx - 1) * tw < W and nty * th >= H and (nty - 1) * th < H
                        assert tw == min(16 if op == 2 else 32, W)              # tiles start on 128-byte lines (resample2d forward: 64)
                        assert 1 <= G <= C and ngroups * G >= C and (ngroups - 1) * G < C
                        assert nwg == B * ntx * nty * ngroups
                        assert 16 * 1024 <= lds <= 64 * 1024 and lds % 256 == 0
                        if B * ntx * nty * C >= 3 * 256:                        # enough work: at least three workgroups per CU
                            assert nwg >= 3 * 256 or G == 1, (op, B, C, H, W, G, nwg)
    assert seen > 1000
    assert L.gfla_big_plane_geometry(0, 1, 64, 256, 176, 256, 176, 4, 4, po) == 0 and out[0] == 1     # configs[1]
    assert L.gfla_big_plane_geometry(3, 1, 64, 256, 176, 256, 176, 4, 4, po) == 0 and out[0] == 1
    assert L.gfla_big_plane_geometry(0, 32, 128, 64, 44, 64, 44, 6, 4, po) == 0 and out[0] == 0      # bench shape: planes in LDS
    assert L.gfla_big_plane_geometry(2, 32, 64, 256, 176, 256, 176, 4, 4, po) == 0 and out[0] == 0   # many planes: row windows
    assert L.gfla_big_plane_geometry(5, 1, 1, 1, 1, 1, 1, 1, 4, po) == -2 and L.gfla_big_plane_geometry(0, 1, 1, 1, 1, 1, 1, 1, 4, None) == -1
    for nwg in (1, 7, 8, 9, 63, 64, 65, 1536, 1537, 2815, 4099):
        img = [L.gfla_xcd_swizzle(b, nwg) for b in range(nwg)]
        assert sorted(img) == list(range(nwg)), nwg
        for x in range(min(8, nwg)):
            mine = [img[b] for b in range(x, nwg, 8)]
            assert mine == list(range(mine[0], mine[0] + len(mine))), (nwg, x)      # contiguous, in launch order
        assert L.gfla_xcd_swizzle(nwg, nwg) == -1 and L.gfla_xcd_swizzle(-1, nwg) == -1


# ------------------------------------------------------------------------------------------------------- tuning keys
CSRC = os.path.join(ROOT, "global_flow_local_attention_amd", "csrc")
RETIRED_KEYS = (19, 43, 49, 52)


def _header_tuning_keys():
    """{GFLA_TUNE_X: value} read from the header's text, not through the parser under test"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gfla_hip.h")).read(), flags=re.S)
    body = re.search(r"enum gfla_tuning_key \{(.*?)\}", text, flags=re.S).group(1)
    items = [item.strip() for item in body.split(",") if item.strip()]
    assert all(re.fullmatch(r"GFLA_TUNE_\w+ = \d+", item) for item in items), items
    return dict((item.split(" = ")[0], int(item.split(" = ")[1])) for item in items)


def _csrc_without_comments():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".inc")):
            text = open(os.path.join(CSRC, name)).read()
            yield name, re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_tuning_keys_of_header_and_sources_agree():
    keys = _header_tuning_keys()
    assert len(set(keys.values())) == len(keys) >= 40 and all(0 <= v < 64 for v in keys.values())     # kTuningKeys = 64
    retired = {name for name in keys if name.startswith("GFLA_TUNE_RETIRED_")}
    assert sorted(keys[name] for name in retired) == list(RETIRED_KEYS)
    assert all(name == "GFLA_TUNE_RETIRED_%d" % keys[name] for name in retired)
    read, calls = set(), 0
    for name, text in _csrc_without_comments():
        if name == "abi.hip":
            assert "constexpr int kTuningKeys = 64;" in text
        for arg in re.findall(r"\btuning\(([^()]*)\)", text):
            if arg == "int key":       # the declaration (gfla_common.h) and the definition (abi.hip)
                assert name in ("gfla_common.h", "abi.hip")
            elif arg == "key":         # tile_channels' parameter; its call sites are checked below
                assert name == "tile_map.h"
            else:
                assert arg in keys, "%s: tuning(%s) does not name an enumerator" % (name, arg)
                read.add(arg)
                calls += 1
        if name == "tile_map.h":
            assert "inline int tile_channels(gfla_tuning_key key," in text
            passed = re.findall(r"\btile_channels\((\w+),", text)
            assert len(passed) == 4 and set(passed) <= set(keys), passed
            read.update(passed)
    assert calls > 80
    assert read == set(keys) - retired, (sorted(set(keys) - retired - read), sorted(read & retired))


def test_set_tuning_rejects_what_is_no_enumerator(gfla):
    from global_flow_local_attention_amd import _lib
    keys = _header_tuning_keys()
    assert {"GFLA_" + name: value for name, value in _lib.TUNING_KEYS.items()} == keys
    for name, value in keys.items():
        assert getattr(gfla, name[len("GFLA_"):]) == getattr(_lib, name[len("GFLA_"):]) == value
    for key in (18, 63, 26, 64, -1):
        assert key not in keys.values()
        with pytest.raises(ValueError):
            gfla.set_tuning(key, 1)
    c_set = _lib.lib().gfla_set_tuning          # the C entry point takes any number: nothing reads 18, nothing stores 64
    assert (c_set(18, 1), c_set(18, 0), c_set(64, 1), c_set(64, 0)) == (0, 1, 0, 0)
    for key in RETIRED_KEYS:
        gfla.set_tuning(key, gfla.set_tuning(key, 1))
    assert gfla.set_tuning(gfla.TUNE_SPLIT, 3) == 0
    assert gfla.set_tuning(gfla.TUNE_SPLIT, 0) == 3
    assert gfla.set_tuning(gfla.TUNE_SPLIT, 0) == 0


def test_tuned_restores_the_previous_values(gfla):
    G, S = gfla.TUNE_G_CAP, gfla.TUNE_SPLIT

    def now(key):
        value = gfla.set_tuning(key, 0)
        gfla.set_tuning(key, value)
        return value

    assert (now(G), now(S)) == (0, 0)
    with gfla.tuned({G: 2, S: 3}):                      # a normal exit
        assert (now(G), now(S)) == (2, 3)
    assert (now(G), now(S)) == (0, 0)
    with pytest.raises(RuntimeError):                   # an exception inside the block
        with gfla.tuned({G: 2, S: 3}):
            raise RuntimeError("a failing case")
    assert (now(G), now(S)) == (0, 0)
    with pytest.raises(ValueError):                     # a key that is no enumerator: the keys set before it come back too
        with gfla.tuned({G: 2, 18: 1}):
            pass
    assert now(G) == 0
    with gfla.tuned({G: 2}):                            # two blocks that set the same key
        with gfla.tuned({G: 5, S: 1}):
            assert (now(G), now(S)) == (5, 1)
        assert (now(G), now(S)) == (2, 0)
    assert (now(G), now(S)) == (0, 0)
    assert gfla.set_tuning(G, 7) == 0                   # a key that is not 0 on entry
    try:
        with gfla.tuned({G: 1}):
            assert now(G) == 1
        assert now(G) == 7
    finally:
        gfla.set_tuning(G, 0)


def test_no_numeric_tuning_key_in_tests_and_tools():
    """every set_tuning call of tests/ and tools/ names its key (this file passes numbers on purpose)"""
    found = []
    for top in ("tests", "tools"):
        for folder, _, files in os.walk(os.path.join(ROOT, top)):
            for name in files:
                path = os.path.join(folder, name)
                if name.endswith(".py") and path != os.path.abspath(__file__):
                    for n, line in enumerate(open(path), 1):
                        if re.search(r"set_tuning\(\s*\d", line):
                            found.append("%s:%d" % (os.path.relpath(path, ROOT), n))
    assert not found, found
