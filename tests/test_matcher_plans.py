"""CPU: the matcher matrix.  tests/golden/matcher_parent_plans.json holds the plan and blob digests (test_plan_digests.digest's form) a build of the
parent commit gave for one graph per path through the ONNX pattern matchers that the older *_parent_plans.json files leave unpinned: the Swin window
and patch-merge regions, the three GroupNorm forms and a GroupNorm in front of a SiLU, both spelling sets of Llama, a decode and an extend step,
both gelu_new forms, BERT's ktrans / scale / unsqueeze spellings and ViT's two unbind forms, in fp32 and fp16.  A change of the matchers that moves a
plan or a weight blob moves a digest here.

A new spelling adds its case to CASES; the file is then rewritten, from a build whose plans are the ones to keep, by

    python tests/test_matcher_plans.py
"""
import itertools
import json
import os
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    from _pkg import load_package
    load_package()

import extend_graphs as EG  # noqa: E402
import gn_graphs as GN  # noqa: E402
import kv_graphs as KG  # noqa: E402
import swin_graphs as SG  # noqa: E402
import test_plan_digests as TPD  # noqa: E402
import vit_graphs as VG  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "matcher_parent_plans.json")
PRECS = ("fp32", "fp16")
ROWS = np.zeros((7, 4 * 32), np.float32)      # the q | k | v rows of the one-attention decode / extend graphs: 2 heads, 1 K / V head, hd 32

# name -> (the model's bytes, the batch)
CASES = {
    # a shifted and an unshifted block per stage, a patch merge between the stages
    "swin_narrow": (lambda: SG.narrow(2), 2),
    # GroupNorm: form a (Reshape -> InstanceNormalization -> Reshape -> Mul -> Add; the way back a constant or Shape(x)), b (the operator, opset 18 and 21),
    # c (InstanceNormalization on the map), a norm in front of a SiLU, and the two models that hold them
    "gn_a_const": (lambda: GN.gn_graph(2, 32, 6, 6, 8, form="instancenorm", back="const"), 2),
    "gn_a_shape_swapped": (lambda: GN.gn_graph(2, 32, 6, 6, 8, form="instancenorm", back="shape", swap=True), 2),
    "gn_b_op18": (lambda: GN.gn_graph(2, 32, 6, 6, 8, form="op18"), 2),
    "gn_b_op21": (lambda: GN.gn_graph(2, 32, 6, 6, 8, form="op21"), 2),
    "gn_c_instance": (lambda: GN.gn_graph(2, 32, 6, 6, 32, form="instance"), 2),
    "gn_silu": (lambda: GN.gn_graph(2, 32, 6, 6, 8, act="silu"), 2),
    "gn_silu_swapped": (lambda: GN.gn_graph(2, 32, 6, 6, 8, act="silu", act_swap=True), 2),
    "resnet50_gn_narrow": (lambda: models.resnet50_gn("N", image=64, classes=10, layers=(1, 1, 1, 1)), 2),
    "vae_decoder_narrow": (lambda: GN.narrow_decoder("N"), 2),
    "vae_decoder_narrow_op18": (lambda: GN.narrow_decoder("N", gn_form="op18"), 2),
    # Llama: the default spellings, and the other set of test_float64_walk_agrees_across_spellings
    "llama_tiny": (lambda: models.llama_tiny(2), 2),
    "llama_tiny_respelled": (lambda: models.llama_tiny(2, norm="op", cast=True, swap=True, rope="gather", mask="where_const"), 2),
    # a decode and an extend step: the narrow model's, and the attention alone
    "narrow_decode": (lambda: KG.narrow(seq=1, past=KG.NARROW_P), KG.NARROW_N),
    "narrow_extend": (lambda: KG.narrow(seq=4, past=KG.NARROW_P), KG.NARROW_N),
    "decode_attn": (lambda: KG.decode_attn_graph(ROWS, 2, 2, 1, 32, 12), 2),
    "extend_attn": (lambda: EG.extend_attn_graph(ROWS, 2, 2, 1, 32, 12, 4), 2),
    # GPT-2: gelu_new with the Pow and with Mul(x, Mul(x, x))
    "gpt2_tiny_gelu_pow": (lambda: models.gpt2_tiny(2, gelu="pow"), 2),
    "gpt2_tiny_gelu_mulmul": (lambda: models.gpt2_tiny(2, gelu="mulmul"), 2),
    # BERT: every ktrans / scale / unsqueeze spelling of its builder
    "bert_tiny": (lambda: models.bert_tiny(2, ktrans="two", scale="div", unsqueeze="two"), 2),
    "bert_tiny_ktrans_one": (lambda: models.bert_tiny(2, ktrans="one"), 2),
    "bert_tiny_scale_mul": (lambda: models.bert_tiny(2, scale="mul"), 2),
    "bert_tiny_unsqueeze_one": (lambda: models.bert_tiny(2, unsqueeze="one"), 2),
    # ViT: q, k, v as three Gathers, and as Split + Squeeze
    "vit_narrow_gather": (lambda: VG.narrow(2, unbind="gather"), 2),
    "vit_narrow_split": (lambda: VG.narrow(2, unbind="split"), 2),
}


def digests(root, names=CASES):
    out = {}
    for name in names:
        mk, batch = CASES[name]
        path = models.write_repo(root, name, mk())
        for prec in PRECS:
            d = TPD.digest(path, batch, {"IE_PRECISION": prec})
            assert "error" not in d, (name, prec, d)
            out[f"{name}/{prec}"] = " ".join(d[k] for k in ("plan", "weights") if k in d)
    return out


def _parent():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_every_case():
    assert sorted(_parent()) == sorted(f"{n}/{p}" for n, p in itertools.product(CASES, PRECS))


@pytest.mark.parametrize("name", sorted(CASES))
def test_parent_plans_are_unchanged(tmp_path, name, engine_lib):
    parent = _parent()
    now = digests(str(tmp_path), [name])
    assert {k: v for k, v in now.items() if v != parent[k]} == {}


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp, open(GOLDEN, "w") as f:
        json.dump(digests(tmp), f, indent=0, sort_keys=True)
        f.write("\n")
