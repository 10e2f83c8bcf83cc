"""Embeddings over the public interfaces (CPU only): POST /embedding and POST /v1/embeddings through
the orchestrator's continuous-batching session, and `mi-cli --embedding` against Engine.embed on the
same tokens.  The servers run the CPU backend with cpu_act f32, like the Engine they are compared
with, so the vectors agree to f32 rounding.

(The orchestrator's streaming endpoint is /chat; /completion answers with one JSON body.  The
interleaving test therefore streams /chat and checks the /completion text of the same prompt.)

Ports: reserved for the life of each server as in test_api_logprobs.py."""
import json
import os
import socket
import subprocess
import time

import httpx
import numpy as np
import pytest

from conftest import REPO, make_model

BIN = os.path.join(REPO, "distributed-llm-pipeline_amd", "bin")
TEXTS = ["The pipeline sends activations", "a stage waits for tokens .", "zeta"]


def reserve_port():
    s = socket.socket()
    s.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    s.bind(("127.0.0.1", 0))
    return s, s.getsockname()[1]


class Orchestrator:
    def __init__(self, *args):
        self.hold, self.port = reserve_port()
        self.proc = subprocess.Popen([os.path.join(BIN, "orchestrator"), "--host", "127.0.0.1",
                                      "--port", str(self.port), *args],
                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        self.url = f"http://127.0.0.1:{self.port}"
        t0 = time.time()
        while time.time() - t0 < 60:
            try:
                httpx.get(self.url + "/health", timeout=1)
                return
            except Exception:
                if self.proc.poll() is not None:
                    self.hold.close()
                    raise RuntimeError(self.proc.stdout.read())
                time.sleep(0.05)
        self.close()
        raise RuntimeError("orchestrator did not come up")

    def close(self):
        self.proc.terminate()
        try:
            self.proc.wait(10)
        except subprocess.TimeoutExpired:
            self.proc.kill()
        self.hold.close()


SERVER_FLAGS = ("-ngl", "0", "-n", "16", "-c", "256", "--mb-size", "2", "--cpu-act", "f32", "--threads", "4")


@pytest.fixture(scope="module")
def tiny_gguf(native, model_dir):
    assert os.path.exists(os.path.join(BIN, "orchestrator")) and os.path.exists(os.path.join(BIN, "mi-cli"))
    path, cfg = make_model(model_dir, "tiny-l3", "Q8_0")
    return path


@pytest.fixture(scope="module")
def srv(tiny_gguf):
    s = Orchestrator("-m", tiny_gguf, *SERVER_FLAGS)
    yield s
    s.close()


@pytest.fixture(scope="module")
def expected(tiny_gguf):
    """tokens of TEXTS and Engine.embed of them: {(pooling, normalize): [vectors]}"""
    from mipipe.engine import Engine
    from mipipe.tokenizer import Tokenizer
    tok = Tokenizer(tiny_gguf)
    assert not tok.add_eos
    toks = [tok.encode_for_embedding(t) for t in TEXTS]
    assert toks == [tok.encode(t, add_bos=tok.add_bos) for t in TEXTS]
    tok.close()
    with Engine(gguf=tiny_gguf, backend="cpu", cpu_act="f32", max_ctx=256, mb_size=2, threads=4) as eng:
        vecs = {(p, n): eng.embed(toks, pooling=p, normalize=n) for p in ("last", "mean", "none") for n in (True, False)}
    return toks, vecs


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-5 * (float(np.abs(b).max()) + 1e-30)


def test_embedding_endpoint(srv, expected):
    toks, vecs = expected
    r = httpx.post(srv.url + "/embedding", json={"content": TEXTS[0]}, timeout=120)
    assert r.status_code == 200, r.text
    j = r.json()
    assert isinstance(j, list) and len(j) == 1 and set(j[0]) == {"index", "embedding"} and j[0]["index"] == 0
    assert close(j[0]["embedding"], vecs[("last", True)][0])          # the default pooling of a file without one
    assert abs(np.linalg.norm(j[0]["embedding"]) - 1.0) < 1e-5
    # a list of three with two slots: batched over rounds, answered in order
    j = httpx.post(srv.url + "/embedding", json={"content": TEXTS, "pooling": "mean"}, timeout=120).json()
    assert [e["index"] for e in j] == [0, 1, 2]
    assert all(close(e["embedding"], v) for e, v in zip(j, vecs[("mean", True)]))
    # embd_normalize -1: the vector as computed
    j = httpx.post(srv.url + "/embedding", json={"content": TEXTS[1], "pooling": "mean", "embd_normalize": -1},
                   timeout=120).json()
    assert close(j[0]["embedding"], vecs[("mean", False)][1])
    assert abs(np.linalg.norm(j[0]["embedding"]) - 1.0) > 1e-2
    # pooling none: one vector per token
    j = httpx.post(srv.url + "/embedding", json={"content": TEXTS[0], "pooling": "none"}, timeout=120).json()
    assert close(j[0]["embedding"], vecs[("none", True)][0]) and len(j[0]["embedding"]) == len(toks[0])


def test_openai_endpoint(srv, expected):
    toks, vecs = expected
    for inp, idx in ((TEXTS[0], [0]), (TEXTS, [0, 1, 2]), (toks[1], [1]), (toks, [0, 1, 2])):
        r = httpx.post(srv.url + "/v1/embeddings", json={"input": inp, "encoding_format": "float"}, timeout=120)
        assert r.status_code == 200, r.text
        j = r.json()
        assert set(j) == {"object", "data", "model", "usage"} and j["object"] == "list" and isinstance(j["model"], str)
        assert [e["index"] for e in j["data"]] == list(range(len(idx)))
        assert all(set(e) == {"object", "index", "embedding"} and e["object"] == "embedding" for e in j["data"])
        for e, i in zip(j["data"], idx):
            assert close(e["embedding"], vecs[("last", True)][i])
        n = sum(len(toks[i]) for i in idx)
        assert j["usage"] == {"prompt_tokens": n, "total_tokens": n}
    j = httpx.post(srv.url + "/v1/embeddings", json={"input": TEXTS[2], "pooling": "mean", "embd_normalize": -1},
                   timeout=120).json()
    assert close(j["data"][0]["embedding"], vecs[("mean", False)][2])


def test_bad_requests(srv):
    post = lambda path, body: httpx.post(srv.url + path, json=body, timeout=120)
    r = post("/v1/embeddings", {"input": "x", "pooling": "none"})
    assert r.status_code == 400 and "none" in r.text
    assert post("/embedding", {"content": "x", "pooling": "none"}).status_code == 200
    for path, key in (("/embedding", "content"), ("/v1/embeddings", "input")):
        assert post(path, {key: "x", "embd_normalize": 1}).status_code == 422
        assert post(path, {key: "x", "embd_normalize": "2"}).status_code == 422
        r = post(path, {key: "x", "pooling": "rank"})
        assert r.status_code == 400 and "rank" in r.text
        r = post(path, {key: "x", "pooling": "max"})
        assert r.status_code == 400 and "max" in r.text
        assert post(path, {key: ""}).status_code == 400
        assert post(path, {key: []}).status_code == 400
        assert post(path, {key: ["x", [1, 2]]}).status_code == 400
        assert post(path, {"prompt": "x"}).status_code == 422
        assert httpx.post(srv.url + path, content="{", headers={"content-type": "application/json"}).status_code == 400
        assert httpx.post(srv.url + path, content="{}", headers={"content-type": "text/plain"}).status_code == 415
        assert httpx.get(srv.url + path).status_code == 405
    r = post("/v1/embeddings", {"input": [1, 2, 10 ** 6]})
    assert r.status_code == 400 and "out of range" in r.text
    r = post("/v1/embeddings", {"input": [5] * 300})
    assert r.status_code == 400 and "300 tokens" in r.text
    assert post("/v1/embeddings", {"input": "x", "encoding_format": "base64"}).status_code == 400
    # the server is still fine
    assert post("/v1/embeddings", {"input": "x"}).status_code == 200


def test_embedding_while_a_generation_streams(srv, expected):
    """An embedding request is answered while a /chat stream is running (tokens arrive before and after
    the answer), its vector is the usual one, and the streamed text equals the one generated alone."""
    toks, vecs = expected
    prompt, n = "The pipeline sends activations to the next", 120
    alone = httpx.post(srv.url + "/completion", json={"prompt": prompt, "n_predict": n}, timeout=120).json()["content"]
    pieces, after = [], 0
    answered = False
    with httpx.stream("POST", srv.url + "/chat", json={"prompt": prompt, "n_predict": n}, timeout=120) as st:
        for line in st.iter_lines():
            if not line.startswith("data: "):
                continue
            ev = json.loads(line[6:])
            if ev["msg_type"] != "token":
                continue
            pieces.append(ev["content"])
            after += answered
            if len(pieces) == 3 and not answered:
                for i in range(3):
                    r = httpx.post(srv.url + "/v1/embeddings", json={"input": TEXTS[i], "pooling": "mean"}, timeout=120)
                    assert r.status_code == 200, r.text
                    assert close(r.json()["data"][0]["embedding"], vecs[("mean", True)][i])
                answered = True
    assert answered and after > 0, (len(pieces), after)
    assert "".join(pieces) == alone


def test_metrics_count_embeddings(srv):
    def counters():
        m = httpx.get(srv.url + "/metrics").text
        get = lambda k: int([ln for ln in m.splitlines() if ln.startswith(k + " ")][0].split()[1])
        return get("mipipe_embedding_requests_total"), get("mipipe_embedding_tokens_total")
    r0, t0 = counters()
    j = httpx.post(srv.url + "/v1/embeddings", json={"input": TEXTS}, timeout=120).json()
    r1, t1 = counters()
    assert r1 == r0 + 1 and t1 == t0 + j["usage"]["prompt_tokens"] > t0


def test_api_key_and_rate_limit_apply(tiny_gguf):
    s = Orchestrator("-m", tiny_gguf, *SERVER_FLAGS, "--api-key", "k", "--rate-limit", "2")
    try:
        assert httpx.post(s.url + "/embedding", json={"content": "x"}, timeout=120).status_code == 401
        h = {"authorization": "Bearer k"}
        assert httpx.post(s.url + "/embedding", json={"content": "x"}, headers=h, timeout=120).status_code == 200
        assert httpx.post(s.url + "/v1/embeddings", json={"input": "x"}, headers=h, timeout=120).status_code == 200
        assert httpx.post(s.url + "/v1/embeddings", json={"input": "x"}, headers=h, timeout=120).status_code == 429
    finally:
        s.close()


def _cli_vectors(args):
    p = subprocess.run([os.path.join(BIN, "mi-cli"), *args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    out = []
    for k, line in enumerate(p.stdout.strip().splitlines()):
        head, _, rest = line.partition(":")
        assert head == f"embedding {k}", line
        out.append(np.array([float(x) for x in rest.split()], np.float32))
    return out


def test_cli_embedding_matches_engine(tiny_gguf, expected, tmp_path):
    toks, vecs = expected
    base = ["-m", tiny_gguf, "-ngl", "0", "-c", "256", "--cpu-act", "f32", "--mb-size", "2", "--threads", "4", "--embedding"]
    got = _cli_vectors(base + ["-p", TEXTS[0]])
    assert len(got) == 1 and np.array_equal(got[0], vecs[("last", True)][0])
    f = tmp_path / "prompts.txt"
    f.write_text("\n".join(TEXTS) + "\n")
    got = _cli_vectors(base + ["-f", str(f), "--pooling", "mean", "--embd-normalize", "-1"])
    assert len(got) == 3 and all(np.array_equal(g, v) for g, v in zip(got, vecs[("mean", False)]))
    got = _cli_vectors(base + ["-p", TEXTS[2], "--pooling", "none"])
    assert len(got) == len(toks[2]) and np.array_equal(np.stack(got), vecs[("none", True)][2])
    p = subprocess.run([os.path.join(BIN, "mi-cli"), *base, "-p", "x", "--pooling", "rank"], capture_output=True, text=True)
    assert p.returncode != 0 and "rank" in p.stderr


def test_eos_is_appended_when_the_file_asks(native, model_dir, expected):
    """A file written with tokenizer.ggml.add_eos_token = true (and pooling_type = 1): the embedding
    text paths run on the text's tokens + EOS and pool by the file's type; token-id input is taken
    as given; generation does not get the EOS."""
    from mipipe.engine import Engine
    from mipipe.tokenizer import Tokenizer
    path, cfg = make_model(model_dir, "tiny-l3", "Q8_0", add_eos=True, pooling_type=1)
    tok = Tokenizer(path)
    assert tok.add_eos and tok.eos >= 0
    plain = tok.encode(TEXTS[0], add_bos=tok.add_bos)
    with_eos = tok.encode_for_embedding(TEXTS[0])
    tok.close()
    assert with_eos == plain + [tok.eos] and expected[0][0] == plain
    with Engine(gguf=path, backend="cpu", cpu_act="f32", max_ctx=256, mb_size=2, threads=4) as eng:
        assert eng.info["pooling"] == "mean"
        want, without = eng.embed([with_eos, plain])
    assert not close(want, without)
    got = _cli_vectors(["-m", path, "-ngl", "0", "-c", "256", "--cpu-act", "f32", "--threads", "4", "--embedding", "-p", TEXTS[0]])
    assert np.array_equal(got[0], want)
    s = Orchestrator("-m", path, *SERVER_FLAGS)
    try:
        j = httpx.post(s.url + "/v1/embeddings", json={"input": TEXTS[0]}, timeout=120).json()
        assert j["usage"]["prompt_tokens"] == len(plain) + 1 and close(j["data"][0]["embedding"], want)
        j = httpx.post(s.url + "/v1/embeddings", json={"input": plain}, timeout=120).json()
        assert j["usage"]["prompt_tokens"] == len(plain) and close(j["data"][0]["embedding"], without)
        c = httpx.post(s.url + "/completion", json={"prompt": TEXTS[0], "n_predict": 2}, timeout=120).json()
        assert c["tokens_evaluated"] == len(plain)
    finally:
        s.close()
