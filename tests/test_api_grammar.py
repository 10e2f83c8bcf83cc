"""The HTTP and command-line surface of constrained output (orchestrator --row-masks, CPU backend,
-ngl 0): grammar, json_schema and response_format on /completion and /chat, and mi-cli --grammar / -j.
The weights are random, so the grammar alone decides the shape of the output."""
import json
import os
import subprocess
import threading

import httpx
import pytest

from test_api import BIN, Orchestrator, native_bins, sse_events, tiny_gguf  # noqa: F401  (fixtures)

PL, PS = "The pipeline sends activations", "Once upon a time"
SERVER = ("-ngl", "0", "-c", "512", "--mb-size", "2", "--micro-batches", "2", "--threads", "2")
YES_NO = 'root ::= "yes" | "no"'
SCHEMA = {"type": "object", "properties": {"count": {"type": "integer"}, "mood": {"enum": ["calm", "wild"]}},
          "required": ["count", "mood"]}


@pytest.fixture(scope="module")
def srv(native_bins, tiny_gguf):
    s = Orchestrator("-m", tiny_gguf, *SERVER, "--row-masks")
    yield s
    s.close()


def _post(s, **body):
    return httpx.post(s.url + "/completion", json=body, timeout=120)


def _cli(tiny_gguf, prompt, n, *extra):
    p = subprocess.run([os.path.join(BIN, "mi-cli"), "-m", tiny_gguf, "-c", "512", "-ngl", "0", "--no-display-prompt",
                        "-p", prompt, "-n", str(n), *extra], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    return p.stdout.decode("utf-8", errors="replace").rstrip("\n")


def _fits(schema, reply):
    """The reply's content is a document of the schema's grammar, or, cut at n_predict, a prefix of one."""
    from mipipe.grammar import Grammar
    st = Grammar(json_schema=schema).state()
    assert st.accept_text(reply["content"]), reply
    if reply["stop_reason"] == "length":
        return None
    assert reply["stop_reason"] == "eog" and st.can_end, reply
    return json.loads(reply["content"])


def test_yes_or_no(srv):
    for extra in (dict(), dict(temperature=1.5, seed=1), dict(temperature=1.5, seed=2)):
        r = _post(srv, prompt=PS, n_predict=16, grammar=YES_NO, **extra).json()
        assert r["content"] in ("yes", "no") and r["stop_reason"] == "eog", r


def test_json_schema_and_response_format(srv):
    docs = []
    for fields in (dict(json_schema=SCHEMA),
                   dict(response_format={"type": "json_schema", "json_schema": {"schema": SCHEMA}}),
                   dict(response_format={"type": "json_schema", "schema": SCHEMA})):
        doc = _fits(SCHEMA, _post(srv, prompt=PS, n_predict=200, **fields).json())
        if doc is not None:
            assert set(doc) == {"count", "mood"} and isinstance(doc["count"], int) and doc["mood"] in ("calm", "wild")
        docs.append(doc)
    assert docs[0] == docs[1] == docs[2]                      # three spellings of one request
    r = _post(srv, prompt=PS, n_predict=200, response_format={"type": "json_object"}).json()
    doc = _fits({"type": "json_object"}, r)
    assert doc is None or isinstance(doc, dict)
    assert r["content"].startswith("{")


def test_constrained_beside_free_requests(srv, tiny_gguf):
    greedy_ref = _cli(tiny_gguf, PL, 24)
    sampled = dict(prompt=PS, n_predict=24, temperature=0.9, seed=99)
    alone = _post(srv, **sampled).json()
    done = {}

    def go(name, **body):
        done[name] = _post(srv, **body).json()

    th = [threading.Thread(target=go, args=("json",), kwargs=dict(prompt=PS, n_predict=60, json_schema=SCHEMA)),
          threading.Thread(target=go, args=("greedy",), kwargs=dict(prompt=PL, n_predict=24)),
          threading.Thread(target=go, args=("sampled",), kwargs=sampled)]
    [t.start() for t in th]
    [t.join() for t in th]
    _fits(SCHEMA, done["json"])
    assert done["greedy"]["content"] == greedy_ref
    assert done["sampled"]["content"] == alone["content"] and done["sampled"]["seed"] == 99


def test_mask_is_cleared_with_the_slot(tiny_gguf, native_bins):
    """One slot: the greedy request after the constrained one runs in the slot it left."""
    s = Orchestrator("-m", tiny_gguf, "-ngl", "0", "-c", "512", "--threads", "2", "--row-masks")
    try:
        r = _post(s, prompt=PS, n_predict=16, grammar=YES_NO).json()
        assert r["content"] in ("yes", "no")
        assert _post(s, prompt=PL, n_predict=24).json()["content"] == _cli(tiny_gguf, PL, 24)
    finally:
        s.close()


def test_chat_streams_the_same_text(srv):
    g = 'root ::= ("alpha" | "beta" | "gamma") " " [0-9]{3}'
    want = _post(srv, prompt=PS, n_predict=32, grammar=g).json()
    assert want["stop_reason"] == "eog" and want["content"].split(" ")[0] in ("alpha", "beta", "gamma")
    with httpx.stream("POST", srv.url + "/chat", json={"prompt": PS, "n_predict": 32, "grammar": g}, timeout=120) as r:
        assert r.status_code == 200
        ev, _ = sse_events(r)
    assert "".join(e["content"] for e in ev if e["msg_type"] == "token") == want["content"]


def test_bad_requests(srv, tiny_gguf, native_bins):
    r = _post(srv, prompt=PS, grammar=YES_NO, json_schema=SCHEMA)
    assert r.status_code == 400 and "one of" in r.text
    r = _post(srv, prompt=PS, json_schema=SCHEMA, response_format={"type": "json_object"})
    assert r.status_code == 400
    r = _post(srv, prompt=PS, grammar='root ::= item\nitem ::= "a" missing')
    assert r.status_code == 400 and 'rule "item"' in r.text and "missing" in r.text
    r = _post(srv, prompt=PS, grammar='root ::= root "a" | "a"')
    assert r.status_code == 400 and "left recursion" in r.text
    # hostile grammars: a parser error in the reply, not a dead server
    for g, what in (('root ::= ("a"?){0,100000}', "too large"), ("root ::= " + "(" * 60000 + '"a"' + ")" * 60000, "nested more than"),
                    ("root ::=" + " n" * 40 + '\nn ::= | "a" | ', "too ambiguous")):
        r = _post(srv, prompt=PS, grammar=g)
        assert r.status_code == 400 and what in r.text and 'rule "root"' in r.text, r.text[:200]
    deep = {"$ref": "#/$defs/d0", "$defs": {**{f"d{i}": {"$ref": f"#/$defs/d{i + 1}"} for i in range(3000)}, "d3000": {"type": "null"}}}
    r = _post(srv, prompt=PS, json_schema=deep)
    assert r.status_code == 400 and "nested" in r.text
    assert srv.proc.poll() is None
    r = _post(srv, prompt=PS, json_schema={"type": "string", "pattern": "a+"})
    assert r.status_code == 400 and "pattern" in r.text
    r = _post(srv, prompt=PS, response_format={"type": "xml"})
    assert r.status_code == 400
    r = httpx.post(srv.url + "/chat", json={"prompt": PS, "grammar": 5}, timeout=30)
    assert r.status_code == 400
    assert _post(srv, prompt=PS, n_predict=4).status_code == 200          # the server is still fine
    plain = Orchestrator("-m", tiny_gguf, "-ngl", "0", "-c", "256", "--row-sampling")
    try:
        for fields in (dict(grammar=YES_NO), dict(json_schema=SCHEMA), dict(response_format={"type": "json_object"})):
            r = _post(plain, prompt=PS, n_predict=2, **fields)
            assert r.status_code == 400 and "--row-masks" in r.text
    finally:
        plain.close()
    spawn = Orchestrator("--spawn-cli", "mi-cli", "-m", tiny_gguf, "-ngl", "0", "-c", "256")
    try:
        r = _post(spawn, prompt=PS, n_predict=2, grammar=YES_NO)
        assert r.status_code == 400 and "spawn-cli" in r.text
    finally:
        spawn.close()


def test_cli_grammar_and_json_schema(tiny_gguf, native_bins, tmp_path):
    g = 'root ::= ("north" | "south") "-" [a-c]{2}'
    members = {f"{w}-{a}{b}" for w in ("north", "south") for a in "abc" for b in "abc"}
    assert _cli(tiny_gguf, PS, 32, "--grammar", g) in members
    f = tmp_path / "g.gbnf"
    f.write_text(g + "\n")
    assert _cli(tiny_gguf, PS, 32, "--grammar-file", str(f), "--temp", "1.2", "--seed", "5") in members
    doc = json.loads(_cli(tiny_gguf, PS, 200, "-j", json.dumps({"type": "object", "properties": {"ok": {"type": "boolean"}},
                                                                "required": ["ok"]})))
    assert set(doc) == {"ok"} and isinstance(doc["ok"], bool)
    for extra, what in ((["--grammar", g, "--perplexity"], "perplexity"), (["--grammar", g, "--embedding"], "embedding"),
                        (["--grammar", g, "--rpc", "127.0.0.1:1"], "rpc"), (["--grammar", g, "--world", "2", "--rank", "0"], "world"),
                        (["--grammar", "root ::= nope"], "nope"), (["-j", '{"type":"string","format":"date"}'], "format"),
                        (["--grammar", g, "-j", "{}"], "one of")):
        p = subprocess.run([os.path.join(BIN, "mi-cli"), "-m", tiny_gguf, "-ngl", "0", "-c", "256", "-p", "x", *extra],
                           capture_output=True, timeout=60)
        assert p.returncode != 0 and what in p.stderr.decode(errors="replace"), (extra, p.stderr[-300:])
