"""The HTTP surface of per-request sampling (orchestrator --row-sampling, CPU backend, -ngl 0): the
llama.cpp-server sampling fields of /completion and /chat reach the request's slot record; a request's
text depends on its own fields and seed, not on the traffic beside it."""
import os
import subprocess
import threading

import httpx
import pytest

from test_api import BIN, Orchestrator, native_bins, sse_events, tiny_gguf  # noqa: F401  (fixtures)

PL, PS = "The pipeline sends activations", "Once upon a time"
SERVER = ("-ngl", "0", "-c", "512", "--mb-size", "2", "--micro-batches", "2", "--threads", "2")


@pytest.fixture(scope="module")
def srv(native_bins, tiny_gguf):
    s = Orchestrator("-m", tiny_gguf, *SERVER, "--row-sampling", "--n-probs", "1")
    yield s
    s.close()


def _post(s, **body):
    return httpx.post(s.url + "/completion", json=body, timeout=120)


def _cli(tiny_gguf, prompt, n):
    out = subprocess.run([os.path.join(BIN, "mi-cli"), "-m", tiny_gguf, "-c", "512", "-ngl", "0", "--no-display-prompt",
                          "-p", prompt, "-n", str(n)], capture_output=True, timeout=120).stdout
    return out.decode("utf-8", errors="replace").rstrip("\n")


def test_seeded_request_is_reproducible_under_traffic(srv):
    """temperature + seed, sent twice while other requests with other settings come and go: the same
    content both times, and the reply echoes the seed; a request without a seed reports the one it got."""
    done = {}

    def go(name, **body):
        done[name] = _post(srv, **body).json()

    sampled = dict(prompt=PS, n_predict=24, temperature=0.9, top_k=40, seed=1234)
    th = [threading.Thread(target=go, args=("long", ), kwargs=dict(prompt=PL, n_predict=60, temperature=1.2, seed=7)),
          threading.Thread(target=go, args=("a", ), kwargs=sampled)]
    [t.start() for t in th]
    th[1].join()
    go("other", prompt=PL, n_predict=5, temperature=0.5)        # takes the slot a just left, with a default seed
    go("b", **sampled)                                          # admitted beside the long request, at another round
    th[0].join()
    go("c", **dict(sampled, seed=1235))
    assert done["a"]["content"] == done["b"]["content"] and done["a"]["tokens_predicted"] == 24
    assert done["a"]["seed"] == done["b"]["seed"] == 1234 and done["long"]["seed"] == 7
    assert done["c"]["content"] != done["a"]["content"]
    assert "seed" in done["other"] and done["other"]["seed"] not in (7, 1234)
    # the reported default seed reproduces that request
    again = _post(srv, prompt=PL, n_predict=5, temperature=0.5, seed=str(done["other"]["seed"])).json()
    assert again["content"] == done["other"]["content"]


def test_greedy_beside_sampled_equals_cli(srv, tiny_gguf):
    ref = _cli(tiny_gguf, PL, 40)
    done = {}

    def go(name, **body):
        done[name] = _post(srv, **body).json()

    th = [threading.Thread(target=go, args=("hot", ), kwargs=dict(prompt=PS, n_predict=40, temperature=1.5, seed=3)),
          threading.Thread(target=go, args=("greedy", ), kwargs=dict(prompt=PL, n_predict=40, temperature=0))]
    [t.start() for t in th]
    [t.join() for t in th]
    assert done["greedy"]["content"] == ref
    assert done["hot"]["content"] != _cli(tiny_gguf, PS, 40)


def test_logit_bias_bans_the_greedy_first_token(srv):
    base = _post(srv, prompt=PS, n_predict=4, n_probs=1).json()
    first = base["completion_probabilities"][0]["id"]
    for bias in ([[first, False]], {str(first): -1000.0}):
        r = _post(srv, prompt=PS, n_predict=4, n_probs=1, logit_bias=bias).json()
        ids = [e["id"] for e in r["completion_probabilities"]]
        assert ids[0] != first and first not in ids, (bias, ids)
    # the chat endpoint takes the fields too
    with httpx.stream("POST", srv.url + "/chat", json=dict(prompt=PS, n_predict=4, logit_bias=[[first, False]]),
                      timeout=120) as resp:
        ev, _ = sse_events(resp)
    assert "".join(e["content"] for e in ev if e["msg_type"] == "token") == r["content"]


def test_bad_values_are_400(srv):
    for body in (dict(logit_bias="x"), dict(logit_bias=[[1]]), dict(logit_bias=[[1, "a"]]), dict(logit_bias=[[10 ** 7, 1.0]]),
                 dict(logit_bias=[[i, 1.0] for i in range(33)]), dict(top_p=0.0), dict(top_p=1.5), dict(min_p=-1),
                 dict(repeat_penalty=0), dict(temperature="hot"), dict(top_k=-2), dict(repeat_last_n=8)):
        r = _post(srv, prompt=PS, n_predict=2, **body)
        assert r.status_code == 400, (body, r.status_code, r.text)
    assert _post(srv, prompt=PS, n_predict=2, repeat_last_n=64).status_code == 200
    assert _post(srv, prompt=PS, n_predict=2, seed=-1, temperature=0.7).status_code == 200   # "pick a seed"


def test_fields_need_the_flag(native_bins, tiny_gguf):
    s = Orchestrator("-m", tiny_gguf, *SERVER)
    try:
        for body in (dict(temperature=0.8), dict(seed=1), dict(logit_bias=[[5, False]]), dict(top_k=40),
                     dict(repeat_penalty=1.1)):
            r = _post(s, prompt=PS, n_predict=2, **body)
            assert r.status_code == 400 and "--row-sampling" in r.text, (body, r.status_code, r.text)
        r = httpx.post(s.url + "/chat", json=dict(prompt=PS, n_predict=2, temperature=0.8), timeout=60)
        assert r.status_code == 400 and "--row-sampling" in r.text
        ok = _post(s, prompt=PS, n_predict=2)
        assert ok.status_code == 200 and "seed" not in ok.json()
    finally:
        s.close()


def test_spawn_cli_rejects_the_fields(native_bins, tiny_gguf):
    s = Orchestrator("--spawn-cli", "mi-cli", "-m", tiny_gguf, "-ngl", "0", "-c", "256")
    try:
        r = _post(s, prompt=PS, n_predict=2, temperature=0.8)
        assert r.status_code == 400 and "spawn-cli" in r.text
    finally:
        s.close()


def test_failed_over_request_continues_its_own_stream(native_bins, tiny_gguf, srv):
    """A stage faults mid-generation: the sampled request is re-admitted into the replacement engine
    with its seed and draw0 = the tokens it has produced, so its text is the fault-free one."""
    import json
    import time
    from test_api import free_port
    body = dict(prompt=PL, n_predict=40, temperature=0.9, top_k=40, seed=1234)
    ref = _post(srv, **body).json()
    port = free_port()
    proc = subprocess.Popen([os.path.join(BIN, "orchestrator"), "--host", "127.0.0.1", "--port", str(port),
                             "-m", tiny_gguf, "-ngl", "0", "-c", "512", "--stages", "2", "--split", "even",
                             "--threads", "2", "--row-sampling"],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                            env={**os.environ, "MIPIPE_FAULT": json.dumps({"stage": 1, "fail_at": 25})})
    url = f"http://127.0.0.1:{port}"
    try:
        t0 = time.time()
        while time.time() - t0 < 60:
            try:
                httpx.get(url + "/health", timeout=1)
                break
            except Exception:
                time.sleep(0.1)
        r = httpx.post(url + "/completion", json=body, timeout=120).json()
        h = httpx.get(url + "/health", timeout=30).json()
        assert h["ok"] and h["engine_restarts"] == 1 and len(h["stages"]) == 1
        assert r["tokens_predicted"] == 40 and r["seed"] == 1234
        assert r["content"] == ref["content"]
    finally:
        proc.terminate()
        proc.wait(timeout=30)
