"""The command-line and HTTP surface of LoRA adapters through the real binaries on the CPU backend
(-ngl 0): mi-cli --lora / --lora-scaled, orchestrator --lora with GET / POST /lora-adapters and the
per-request "lora" field.  The weights are random; the adapter is large enough to change the greedy
text."""
import os
import subprocess
import threading

import httpx
import pytest

from lora_helpers import make_adapter
from test_api import BIN, Orchestrator, native_bins, tiny_gguf  # noqa: F401  (fixtures)

PROMPT = "The pipeline sends activations"
N = 12
CPU = ("-ngl", "0", "-c", "256", "--threads", "2", "--cpu-act", "f32")


@pytest.fixture(scope="module")
def adapters(native, model_dir, tiny_gguf):
    from mipipe.models.config import CONFIGS
    cfg = CONFIGS["tiny-l3"]
    pa, _ = make_adapter(model_dir, tiny_gguf, cfg, seed=71)
    pb, _ = make_adapter(model_dir, tiny_gguf, cfg, seed=72, ranks=(3, 8))
    return pa, pb


def _cli(tiny_gguf, *extra, ok=True):
    p = subprocess.run([os.path.join(BIN, "mi-cli"), "-m", tiny_gguf, *CPU, "--no-display-prompt", "-p", PROMPT, "-n", str(N),
                        *extra], capture_output=True, timeout=180)
    if ok:
        assert p.returncode == 0, p.stderr.decode(errors="replace")
        return p.stdout.decode("utf-8", errors="replace").rstrip("\n")
    assert p.returncode != 0
    return p.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def texts(native_bins, tiny_gguf, adapters):
    return dict(base=_cli(tiny_gguf), a=_cli(tiny_gguf, "--lora", adapters[0]))


def test_cli_lora_changes_the_text_and_matches_the_python_engine(native, tiny_gguf, adapters, texts):
    from mipipe.engine import Engine
    from mipipe.tokenizer import Tokenizer
    assert texts["a"] != texts["base"]
    tok = Tokenizer(tiny_gguf)
    prompt = tok.encode(PROMPT, add_bos=tok.add_bos)
    with Engine(gguf=tiny_gguf, backend="cpu", cpu_act="f32", max_ctx=256, threads=2, lora_adapters=1) as eng:
        assert eng.load_adapter(adapters[0]) == 0
        eng.start([prompt], adapters=[(0, 1.0)])
        eng.decode(N - 1)
        out = eng.tokens()[0][:N]
    stop = [i for i, t in enumerate(out) if t in (tok.eos, tok.eot)]
    out = out[:stop[0]] if stop else out
    assert tok.decode(out) == texts["a"]


def test_cli_scale_zero_is_the_base_model(tiny_gguf, adapters, texts):
    assert _cli(tiny_gguf, "--lora-scaled", adapters[0], "0") == texts["base"]
    assert _cli(tiny_gguf, "--lora-scaled", adapters[0], "1.0") == texts["a"]


def test_cli_refusals(tiny_gguf, adapters):
    assert "exactly one adapter" in _cli(tiny_gguf, "--lora", adapters[0], "--lora", adapters[1], ok=False)
    assert "--rpc" in _cli(tiny_gguf, "--lora", adapters[0], "--rpc", "127.0.0.1:1", ok=False)
    assert "--world" in _cli(tiny_gguf, "--lora", adapters[0], "--world", "2", "--rank", "0", ok=False)
    assert "bad scale" in _cli(tiny_gguf, "--lora-scaled", adapters[0], "much", ok=False)
    assert "general.type" in _cli(tiny_gguf, "--lora", tiny_gguf, ok=False)   # a model is not an adapter


def _post(s, **body):
    return httpx.post(s.url + "/completion", json=dict(prompt=PROMPT, n_predict=N, **body), timeout=180)


def test_server_per_request_adapters(native_bins, tiny_gguf, adapters, texts):
    """Two adapters, --lora-init-without-apply: GET lists them at scale 0; a request with the "lora" field
    gets the adapter's text while a concurrent one without it gets the base text; POST sets the default."""
    s = Orchestrator("-m", tiny_gguf, *CPU, "--mb-size", "2", "--lora", adapters[0], "--lora", adapters[1],
                     "--lora-init-without-apply")
    try:
        r = httpx.get(s.url + "/lora-adapters", timeout=30)
        assert r.status_code == 200
        assert r.json() == [{"id": 0, "path": adapters[0], "scale": 0.0}, {"id": 1, "path": adapters[1], "scale": 0.0}]
        out = {}

        def ask(key, **body):
            out[key] = _post(s, **body)

        th = [threading.Thread(target=ask, args=("a",), kwargs=dict(lora=[{"id": 0, "scale": 1}])),
              threading.Thread(target=ask, args=("base",))]
        [t.start() for t in th]
        [t.join() for t in th]
        assert out["a"].status_code == 200 and out["base"].status_code == 200
        assert out["a"].json()["content"] == texts["a"]
        assert out["base"].json()["content"] == texts["base"]
        # an entry at scale 0 beside the chosen one is fine; the explicit empty list is the base model
        assert _post(s, lora=[{"id": 1, "scale": 0}, {"id": 0, "scale": 1.0}]).json()["content"] == texts["a"]
        assert _post(s, lora=[]).json()["content"] == texts["base"]
        # the 400s
        for bad, needle in (([{"id": 7, "scale": 1}], "unknown adapter id"),
                            ([{"id": 0, "scale": 1}, {"id": 1, "scale": 0.5}], "more than one"),
                            ({"id": 0}, "expected a list"), ([{"scale": 1}], "id")):
            r = _post(s, lora=bad)
            assert r.status_code == 400 and needle in r.text, (bad, r.status_code, r.text)
        r = httpx.post(s.url + "/lora-adapters", json=[{"id": 0, "scale": 1}, {"id": 1, "scale": 1}], timeout=30)
        assert r.status_code == 400 and "more than one" in r.text
        # POST the default: requests without the field now get adapter 0
        r = httpx.post(s.url + "/lora-adapters", json=[{"id": 0, "scale": 1.0}], timeout=30)
        assert r.status_code == 200 and [a["scale"] for a in r.json()] == [1.0, 0.0]
        assert _post(s).json()["content"] == texts["a"]
        assert _post(s, lora=[{"id": 0, "scale": 0}]).json()["content"] == texts["base"]   # the field overrides it
        h = httpx.get(s.url + "/health", timeout=30).json()
        assert [a["id"] for a in h["lora_adapters"]] == [0, 1]
    finally:
        s.close()


def test_server_single_lora_is_the_default_and_plain_server_refuses(native_bins, tiny_gguf, adapters, texts):
    s = Orchestrator("-m", tiny_gguf, *CPU, "--lora", adapters[0])
    try:
        assert httpx.get(s.url + "/lora-adapters", timeout=30).json() == [{"id": 0, "path": adapters[0], "scale": 1.0}]
        assert _post(s).json()["content"] == texts["a"]
    finally:
        s.close()
    plain = Orchestrator("-m", tiny_gguf, *CPU)
    try:
        r = _post(plain, lora=[{"id": 0, "scale": 1}])
        assert r.status_code == 400 and "--lora" in r.text
        assert httpx.get(plain.url + "/lora-adapters", timeout=30).json() == []
        r = httpx.post(plain.url + "/lora-adapters", json=[{"id": 0, "scale": 1}], timeout=30)
        assert r.status_code == 400 and "--lora" in r.text
    finally:
        plain.close()
