"""The one check of a refused load, for every plan test: DescribeModel raises, the text holds the caller's fragments (the node and the rule), and the
WHOLE text is the one tests/golden/refusal_texts.json holds for this (model, batch, precision, environment).  A refusal the golden file does not know
fails.

The key is the sha256 of the model's bytes, the batch, the precision and the sorted environment items: the graph builders are seeded, so a key depends
on neither the order of the tests nor their names.

Recording is the only way the golden file is written, from a build whose texts are the ones to keep:

    python tests/refusals.py                                (= IE_RECORD_REFUSALS=1 pytest over the plan tests: rewrites the file)
"""
from __future__ import annotations

import hashlib
import json
import os
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "refusal_texts.json")
RECORD = "IE_RECORD_REFUSALS"
_golden = None


def key(model_bytes: bytes, batch: int, prec: str, env: dict) -> str:
    h = hashlib.sha256(model_bytes)
    h.update(json.dumps([int(batch), prec, sorted((k, str(v)) for k, v in env.items())]).encode())
    return h.hexdigest()


def _texts() -> dict:
    global _golden
    if _golden is None:
        _golden = {}
        if os.path.exists(GOLDEN):
            with open(GOLDEN) as f:
                _golden = json.load(f)
    return _golden


def _record(k: str, text: str) -> None:
    texts = _texts()
    assert texts.get(k, text) == text, f"one key, two texts:\n{texts[k]}\n{text}"
    texts[k] = text
    with open(GOLDEN, "w") as f:
        json.dump(texts, f, indent=0, sort_keys=True)
        f.write("\n")


def refused(path_or_model, batch, monkeypatch, *fragments, prec="fp32", match=None, **env) -> str:
    """The load of a model (its bytes, or the version directory models.write_repo returned) is refused with a RuntimeError whose text holds every
    fragment, matches the regex `match` where one is given (pytest.raises' own search), and equals the golden text.  -> the text"""
    from engine_run import describe_model
    from gpu_ai_inference_server_amd.modelgen import models
    with tempfile.TemporaryDirectory() as root:
        if isinstance(path_or_model, (bytes, bytearray)):
            model, path = bytes(path_or_model), models.write_repo(root, "bad", bytes(path_or_model))
        else:
            path = str(path_or_model)
            with open(os.path.join(path, "model.onnx"), "rb") as f:
                model = f.read()
        with pytest.raises(RuntimeError, match=match) as e:
            describe_model(path, batch, monkeypatch, prec, **env)
    text = str(e.value)
    for fragment in fragments:
        assert fragment in text, text
    assert path not in text, text              # (a text with the model's directory in it could not be pinned)
    k = key(model, batch, prec, env)
    if os.environ.get(RECORD) == "1":
        _record(k, text)
        return text
    assert k in _texts(), f"no golden text for this refusal (record it: python tests/refusals.py): {text}"
    assert _texts()[k] == text, f"the refusal text moved:\n  golden: {_texts()[k]}\n  now:    {text}"
    return text


if __name__ == "__main__":
    import glob
    import sys
    if os.path.exists(GOLDEN):
        os.remove(GOLDEN)
    os.environ[RECORD] = "1"
    sys.exit(pytest.main(["-q", "-m", "not gpu", "-p", "no:cacheprovider", *sorted(glob.glob(os.path.join(HERE, "test_*_plan.py"))), *sys.argv[1:]]))
