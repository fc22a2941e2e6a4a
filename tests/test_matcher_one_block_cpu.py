"""The matcher's host side states its residual block once: one weight type per precision (AttnBlock / F32Block in airslam_amd/csrc/airfe_host.h), one loader for what
the blocks of LightGlue's two halves and of SuperGlue share (airfe_load.hip), one runner per precision for a block (airfe_match.hip).  Source text with the comments
stripped, as tests/test_debug_hooks_one_holder_cpu.py reads it: a second copy of a launch sequence, of a loader stanza or of a constant shows up here as a count."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "airslam_amd", "csrc")


def _code(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)      # comments name calls; only code makes them


def test_no_parallel_field_set_for_the_cross_half():
    for name in sorted(os.listdir(CSRC)):
        if not os.path.isfile(os.path.join(CSRC, name)):
            continue
        for word in ("cqk", "cffn0", "cffn3", "cln_g", "cln_b"):
            assert not re.search(r"\b%s\b" % word, _code(name)), (name, word)


@pytest.mark.parametrize("call", ["launch_attention32(", "launch_lg_blockf(", "launch_ln_gelu(", "launch_ln_gelu_f32(", "launch_sg_sinkhorn(", "launch_sg_decode(",
                                  "launch_attention_f32("])
def test_each_block_launch_is_stated_once(call):
    assert len(re.findall(r"(?<![A-Za-z0-9_])" + re.escape(call), _code("airfe_match.hip"))) == 1


def test_one_fp32_linear_and_one_similarity_helper():
    assert len(re.findall(r"\bGemmF32Args\s+\w+\s*;", _code("airfe_match.hip"))) <= 2


def test_keypoint_normalisation_constants_are_computed_once():
    assert _code("airfe_match.hip").count("std::max(c->cfg.image_width, c->cfg.image_height)") == 1


def test_one_loader_for_what_the_blocks_share():
    text = _code("airfe_load.hip")
    assert len(re.findall(r"(?<![A-Za-z0-9_])make_ffn0_folded\(", text)) == 2      # its definition and ONE call
    assert text.count('".ffn.3"') == 1 and text.count('".mlp.3"') == 1
    assert text.count("(f & 63) * 4 + (f >> 6)") == 1
