"""Host-side checks of the two refusals that guard the element-wise kernels, none of which needs a GPU:
the dispatcher that tools/gen_h16.py generates refuses both mixes of the two 16-bit types in every entry with a src_dtype parameter and
is otherwise what it was; every entry of csrc/eltwise.hip checks its dtype (and the activation entries their act) before it launches;
ops.py names the offending tensor before any call."""
import importlib.util
import os
import re

import pytest
import torch

from semantic_pyramid_for_image_generation_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC_ENTRIES = ["sp_ingest_image", "sp_augment_ingest", "sp_augment_ingest_gated", "sp_augment_geom_ingest", "sp_augment_cmat_ingest"]
STRUCT_ENTRIES = {"sp_conv2d_general", "sp_conv2d_igemm", "sp_conv2d_route"}


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("gen_h16", os.path.join(ROOT, "tools", "gen_h16.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = str(tmp_path_factory.mktemp("gen_h16"))
    gen.main(out)
    text = open(os.path.join(out, "dispatch_h16.cpp")).read()
    bodies = {m.group(1): m.group(3) for m in re.finditer(r'^extern "C" (?:int|const char\*) (sp_\w+)\(([^)]*)\) \{\n(.*?)^\}\n', text, flags=re.S | re.M)}
    return gen, out, text, bodies


def test_every_entry_with_a_source_type_refuses_both_mixes(generated):
    gen, _, _, bodies = generated
    protos = {name: [p for _, p in params] for _, name, params in gen.prototypes() if name not in gen.SHARED}
    assert sorted(n for n, p in protos.items() if "src_dtype" in p) == sorted(SRC_ENTRIES)
    for name in SRC_ENTRIES:
        lines = bodies[name].strip().split("\n")
        assert len(lines) == 4, (name, lines)
        assert lines[0].strip() == ('if (dtype == SP_F16 && src_dtype == SP_BF16) { sp_set_error("%s: an SP_BF16 source needs SP_BF16 or SP_F32 '
                                    'storage"); return SP_ERR_UNSUPPORTED; }' % name)
        assert lines[1].strip().startswith("if (dtype == SP_F16) return %s__h16(" % name)           # only after the refusal
        assert "(src_dtype == SP_F16 ? SP_BF16 : src_dtype)" in lines[1] and lines[1].count("SP_BF16") == 2          # src and dtype renamed
        assert lines[2].strip() == ('if (src_dtype == SP_F16) { sp_set_error("%s: an SP_F16 source needs SP_F16 storage"); return '
                                    'SP_ERR_UNSUPPORTED; }' % name)
        assert lines[3].strip() == "return %s__b16(%s);" % (name, ", ".join(protos[name]))


def test_no_other_entry_of_the_dispatcher_changed(generated):
    gen, out, text, bodies = generated
    protos = {name: [p for _, p in params] for _, name, params in gen.prototypes() if name not in gen.SHARED}
    assert set(bodies) == set(protos) and len(protos) > 100
    for name, pn in protos.items():
        if name in SRC_ENTRIES:
            continue
        body = bodies[name]
        assert "SP_ERR_UNSUPPORTED" not in body and "sp_set_error" not in body, name
        lines = body.strip().split("\n")
        assert lines[-1].strip() == "return %s__b16(%s);" % (name, ", ".join(pn)), name
        if name in STRUCT_ENTRIES:
            assert "%s__h16(&q, " % name in body
        elif "dtype" in pn:
            h = ", ".join("SP_BF16" if p == "dtype" else p for p in pn)
            assert [ln.strip() for ln in lines] == ["if (dtype == SP_F16) return %s__h16(%s);" % (name, h), lines[-1].strip()], name
        else:
            assert len(lines) == 1, name
    for tag in ("b16", "h16"):
        renames = open(os.path.join(out, "rename_%s.h" % tag)).read()
        assert all("#define %s %s__%s\n" % (n, n, tag) in renames for n in protos)
    assert text.count("SP_ERR_UNSUPPORTED") == 2 * len(SRC_ENTRIES)


def _entries(path):
    """name -> body of every extern "C" entry of a kernel source."""
    text = open(path).read()
    return {m.group(1): m.group(2) for m in re.finditer(r'^extern "C" int (sp_\w+)\([^{]*\{\n(.*?)^\}\n', text, flags=re.S | re.M)}


def test_every_eltwise_entry_checks_its_storage_type_before_it_launches():
    path = os.path.join(ROOT, "semantic_pyramid_for_image_generation_amd", "csrc", "eltwise.hip")
    entries = _entries(path)
    typed = [n for n, b in entries.items() if "dtype" in b]
    assert sorted(typed) == sorted(["sp_ingest_image", "sp_ingest_image_bwd", "sp_mask_concat", "sp_mask_mul_2d", "sp_act_fwd", "sp_act_bwd",
                                    "sp_scale_add", "sp_rescale_bias", "sp_scale_add_bwd", "sp_permute_chw_hwc", "sp_channel_sum"])
    for name in typed:
        body = entries[name]
        check = 'SP_CHECK_DTYPE(dtype, "%s");' % name
        assert body.count(check) == 1 and body.index(check) < body.index("hipLaunchKernelGGL"), name
        if name in ("sp_act_fwd", "sp_act_bwd"):
            act = 'SP_CHECK_ACT(act, "%s");' % name
            assert body.count(act) == 1 and body.index(act) < body.index("hipLaunchKernelGGL"), name
    text = open(path).read()
    assert re.search(r"#define SP_CHECK_DTYPE\(dtype, name\).*\(dtype\) != SP_F32 && \(dtype\) != SP_BF16.*\\\n.*return SP_ERR_UNSUPPORTED", text)
    assert re.search(r"#define SP_CHECK_ACT\(act, name\).*\(act\) < SP_ACT_NONE \|\| \(act\) > SP_ACT_TANH.*\\\n.*return SP_ERR_UNSUPPORTED", text)
    header = open(_lib.HEADER).read()
    assert "SP_ERR_UNSUPPORTED" in header[header.index("Glue: image ingest"):header.index("int sp_ingest_image(")]


def test_ops_names_the_image_before_any_call():
    bf, hf, f32 = torch.bfloat16, torch.float16, torch.float32
    img = {dt: torch.zeros(1, 3, 2, 2, dtype=dt) for dt in (bf, hf, f32)}
    for src, dst in ((bf, hf), (hf, bf)):
        with pytest.raises(_lib.SempyrError, match="cannot be ingested"):
            ops._ingest_src_dtype(img[src], dst)
    assert ops._ingest_src_dtype(img[f32], hf) == _lib.SP_F32 and ops._ingest_src_dtype(img[f32], bf) == _lib.SP_F32
    assert ops._ingest_src_dtype(img[hf], hf) == _lib.SP_F16 and ops._ingest_src_dtype(img[bf], bf) == _lib.SP_BF16
    assert ops._ingest_src_dtype(img[bf], f32) == _lib.SP_BF16      # the plain compilation reads a bf16 source into fp32 storage
    src = open(ops.__file__).read()
    assert src.count("_ingest_src_dtype(img, dtype)") == 3 and "sp_dtype(img.dtype), sn" not in src      # plain, pair and augmenting paths
