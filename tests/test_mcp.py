"""MCP stdio server tests: JSON-RPC protocol + tool round-trips against the
shared SQLite file (reference: src/mcp tests pattern)."""
import json
import os
import tempfile

import pytest

from room_amd.db import LockedDb
from room_amd.mcp.server import McpServer


@pytest.fixture
def mcp(db):
    nudged = []
    srv = McpServer(LockedDb(db), nudge=lambda wid: nudged.append(wid) or True)
    srv._nudged = nudged
    return srv


def call(srv, name, args, mid=1):
    resp = srv.handle({"jsonrpc": "2.0", "id": mid, "method": "tools/call",
                       "params": {"name": name, "arguments": args}})
    assert "result" in resp, resp
    payload = json.loads(resp["result"]["content"][0]["text"])
    return payload


def test_initialize_and_list(mcp):
    init = mcp.handle({"jsonrpc": "2.0", "id": 0, "method": "initialize",
                       "params": {}})
    assert init["result"]["serverInfo"]["name"] == "room-amd"
    lst = mcp.handle({"jsonrpc": "2.0", "id": 1, "method": "tools/list"})
    tools = lst["result"]["tools"]
    names = {t["name"] for t in tools}
    assert len(tools) >= 30
    assert {"room_create_room", "room_announce", "room_recall",
            "room_delegate_task", "room_modify_skill"} <= names
    # every tool has a schema
    assert all("inputSchema" in t for t in tools)


def test_room_tools_round_trip(mcp):
    out = call(mcp, "room_create_room", {"name": "mcp-room", "goal": "g",
                                         "worker_model": "stub"})
    rid = out["room_id"]
    status = call(mcp, "room_get_status", {"room_id": rid})
    assert status["room"] == "mcp-room"
    w = call(mcp, "room_create_worker", {"room_id": rid, "name": "e",
                                         "role": "executor"})
    d = call(mcp, "room_delegate_task", {"room_id": rid, "description": "do",
                                         "worker_id": w["worker_id"]})
    assert mcp._nudged == [w["worker_id"]]
    tree = call(mcp, "room_goal_tree", {"room_id": rid})
    assert any(g["assigned_worker_id"] == w["worker_id"] for g in tree)


def test_quorum_tools(mcp):
    rid = call(mcp, "room_create_room", {"name": "qr", "worker_model": "stub"})["room_id"]
    w = call(mcp, "room_create_worker", {"room_id": rid, "name": "v",
                                         "role": "guardian"})
    d = call(mcp, "room_announce", {"room_id": rid, "proposal": "big",
                                    "decision_type": "strategy"})
    assert d["status"] == "announced"
    o = call(mcp, "room_object", {"decision_id": d["decision_id"],
                                  "worker_id": w["worker_id"], "reason": "no"})
    assert o["status"] == "objected"


def test_memory_and_skill_tools(mcp):
    rid = call(mcp, "room_create_room", {"name": "mr", "worker_model": "stub"})["room_id"]
    call(mcp, "room_remember", {"room_id": rid, "name": "fact",
                                "content": "the answer is 42"})
    hits = call(mcp, "room_recall", {"room_id": rid, "query": "answer"})
    assert hits and hits[0]["name"] == "fact"
    s = call(mcp, "room_create_skill", {"room_id": rid, "name": "recipe",
                                        "content": "v1"})
    wid = call(mcp, "room_create_worker", {"room_id": rid, "name": "m",
                                           "role": "analyst"})["worker_id"]
    m = call(mcp, "room_modify_skill", {"room_id": rid, "worker_id": wid,
                                        "skill_id": s["skill_id"],
                                        "content": "v2"})
    r = call(mcp, "room_revert_modification", {"audit_id": m["audit_id"]})
    assert r["reverted"]


def test_task_and_wallet_tools(mcp):
    rid = call(mcp, "room_create_room", {"name": "tw", "worker_model": "stub"})["room_id"]
    t = call(mcp, "room_create_task", {"name": "nightly", "prompt": "p",
                                       "cron_expression": "0 2 * * *",
                                       "room_id": rid})
    tasks = call(mcp, "room_list_tasks", {"room_id": rid})
    assert any(x["id"] == t["task_id"] for x in tasks)
    addr = call(mcp, "room_wallet_address", {"room_id": rid})
    assert addr["address"].startswith("0x")
    ident = call(mcp, "room_register_identity", {"room_id": rid})
    assert ident["agent_uri"].startswith("data:application/json;base64,")


def test_watch_path_validation(mcp):
    bad = call(mcp, "room_watch_path", {"path": "/etc/passwd"})
    assert "error" in bad
    bad2 = call(mcp, "room_watch_path", {"path": "~/.ssh/config"})
    assert "error" in bad2
    ok = call(mcp, "room_watch_path", {"path": "~/projects/data"})
    assert "watch_id" in ok


def test_unknown_tool_and_method(mcp):
    resp = mcp.handle({"jsonrpc": "2.0", "id": 5, "method": "tools/call",
                       "params": {"name": "nope", "arguments": {}}})
    assert resp["error"]["code"] == -32602
    resp = mcp.handle({"jsonrpc": "2.0", "id": 6, "method": "bogus"})
    assert resp["error"]["code"] == -32601


def test_parity_surface_tools(mcp):
    """The reference's full 76-tool surface: detail/config/forget/session/
    webhook/resources tools round-trip (mcp/tools/* parity)."""
    out = call(mcp, "room_create_room", {"name": "parity", "goal": "g",
                                         "worker_model": "stub"})
    rid = out["room_id"]

    # decision detail with votes
    ann = call(mcp, "room_announce", {"room_id": rid, "proposal": "d1",
                                      "decision_type": "custom"})
    did = ann["decision_id"]
    w0 = call(mcp, "room_create_worker", {"room_id": rid, "name": "voter",
                                          "role": "executor"})
    call(mcp, "room_object", {"decision_id": did,
                              "worker_id": w0["worker_id"], "reason": "nope"})
    detail = call(mcp, "room_decision_detail", {"decision_id": did})
    assert detail["id"] == did and detail["status"] == "objected"
    assert "votes" in detail

    # skills: activate / deactivate / delete
    sk = call(mcp, "room_create_skill", {"room_id": rid, "name": "s1",
                                         "content": "recipe"})
    sid = sk["skill_id"]
    assert call(mcp, "room_activate_skill", {"skill_id": sid})["activated"]
    assert call(mcp, "room_deactivate_skill", {"skill_id": sid})["deactivated"]
    assert call(mcp, "room_delete_skill", {"skill_id": sid})["deleted"]

    # configure room merges config
    cfg = call(mcp, "room_configure_room",
               {"room_id": rid, "config": {"threshold": "unanimous"}})
    assert cfg["config"]["threshold"] == "unanimous"

    # credentials get returns the decrypted value
    call(mcp, "room_set_credential", {"room_id": rid, "name": "api_key",
                                      "value": "sk-123"})
    got = call(mcp, "room_get_credential", {"room_id": rid, "name": "api_key"})
    assert got["value"] == "sk-123"

    # memory list + forget
    m = call(mcp, "room_remember", {"room_id": rid, "name": "fact",
                                    "content": "water is wet"})
    lst = call(mcp, "room_memory_list", {"room_id": rid})
    assert any(e["name"] == "fact" for e in lst)
    fg = call(mcp, "room_forget", {"entity_id": m["entity_id"]})
    assert fg["forgot"] == "fact"
    assert not any(e["name"] == "fact"
                   for e in call(mcp, "room_memory_list", {"room_id": rid}))

    # identity get (wallet auto-created with the room)
    ident = call(mcp, "room_identity_get", {"room_id": rid})
    assert ident["address"].startswith("0x")

    # invites fail gracefully offline
    inv = call(mcp, "room_invite_create", {"room_id": rid})
    assert "error" in inv

    # watch pause/resume (the allowlist admits home and the temp directory,
    # wherever TMPDIR puts it)
    watched = os.path.join(tempfile.gettempdir(), "x")
    w = call(mcp, "room_watch_path", {"room_id": rid, "path": watched,
                                      "action_prompt": "check"})
    call(mcp, "room_pause_watch", {"watch_id": w["watch_id"]})
    call(mcp, "room_resume_watch", {"watch_id": w["watch_id"]})

    # task session reset + webhook url + run-now fallback
    task = call(mcp, "room_create_task",
                {"name": "t1", "prompt": "p", "room_id": rid,
                 "trigger_type": "manual"})
    tid = task["task_id"]
    assert "reset" in call(mcp, "room_reset_session", {"task_id": tid})
    url = call(mcp, "room_webhook_url", {"task_id": tid,
                                         "generate_if_missing": True})
    assert "/api/hooks/task/" in url["url"]
    run = call(mcp, "room_run_task", {"task_id": tid})
    assert "started" in run or "queued" in run

    # wallet balance (offline → structured error/zero) + topup fallback
    bal = call(mcp, "room_wallet_balance", {"room_id": rid})
    assert isinstance(bal, dict)
    top = call(mcp, "room_wallet_topup", {"room_id": rid, "amount": 25})
    assert "onramp_url" in top or top["address"].startswith("0x")

    # resources
    res = call(mcp, "room_resources", {})
    assert res["cpus"] >= 1 and "summary" in res

    # the full surface is now >= the reference's 76 tools
    lst = mcp.handle({"jsonrpc": "2.0", "id": 9, "method": "tools/list"})
    assert len(lst["result"]["tools"]) >= 90


def test_reference_tool_name_aliases(mcp):
    """Every quoroom_* tool name the reference MCP server registers
    (src/mcp/server.ts, 76 tools) resolves here, so clients configured
    against the reference work unchanged."""
    names = set(mcp.tools)
    ref_suffixes = ["create_room", "list_rooms", "propose", "vote",
                    "delegate_task", "remember", "recall", "schedule",
                    "self_mod_history", "wallet_address", "browser",
                    "inbox_reply", "export_worker_prompts", "webhook_url"]
    for s in ref_suffixes:
        assert f"quoroom_{s}" in names, s
    assert sum(1 for n in names if n.startswith("quoroom_")) == 76
    # aliases execute the same handler
    out = call(mcp, "quoroom_create_room", {"name": "alias-room"})
    assert out["room_id"]
    rooms = call(mcp, "quoroom_list_rooms", {})
    assert any(r["name"] == "alias-room" for r in rooms)


def _all_tools(mcp):
    resp = mcp.handle({"jsonrpc": "2.0", "id": 7, "method": "tools/list",
                       "params": {}})
    return resp["result"]["tools"]


def test_tool_registry_integrity(mcp):
    """Every registered tool exposes a valid MCP tool descriptor: unique
    name, non-empty description, object input schema whose required keys
    exist in properties (the contract clients introspect)."""
    tools = _all_tools(mcp)
    assert len(tools) == len({t["name"] for t in tools})
    for t in tools:
        assert t["name"] and t["description"], t["name"]
        schema = t["inputSchema"]
        assert schema["type"] == "object", t["name"]
        props = schema.get("properties", {})
        for req in schema.get("required", []):
            assert req in props, f"{t['name']}: required {req} not in properties"
        for pname, pdef in props.items():
            assert pdef.get("type") in ("string", "integer", "boolean",
                                        "number", "array", "object"), \
                f"{t['name']}.{pname}"


def test_unknown_tool_and_malformed_args(mcp):
    resp = mcp.handle({"jsonrpc": "2.0", "id": 8, "method": "tools/call",
                       "params": {"name": "room_no_such_tool",
                                  "arguments": {}}})
    assert "error" in resp or resp["result"].get("isError")
    # a tool with missing required args returns a tool error, not a crash
    resp2 = mcp.handle({"jsonrpc": "2.0", "id": 9, "method": "tools/call",
                        "params": {"name": "room_create_room",
                                   "arguments": {}}})
    assert resp2 is not None


def test_every_tool_smoke_callable(mcp):
    """Call EVERY registered tool once with schema-synthesized minimal
    arguments: each must return a JSON-RPC result (ok or a structured tool
    error) — never a handler crash without a response. Guards all ~170
    handlers against signature drift."""
    from room_amd.core import room as room_mod
    from room_amd.db import queries as q

    with mcp.ldb as db:
        r = room_mod.create_room(db, "smoke-room", goal="g",
                                 worker_model="stub")
        room_id = r["id"]
        worker_id = r["queen_worker_id"]
        g = q.create_goal(db, room_id, "smoke goal")
        d = q.create_decision(db, room_id, worker_id, "smoke d", "low_impact")
        ent = q.create_entity(db, "smoke entity", room_id=room_id,
                              observations=["obs"])
        task = q.create_task(db, "smoke task", "do", trigger_type="manual",
                             room_id=room_id)

    known_ids = {"room_id": room_id, "worker_id": worker_id,
                 "target_worker_id": worker_id, "goal_id": g["id"],
                 "decision_id": d["id"], "entity_id": ent["id"],
                 "task_id": task["id"], "parent_goal_id": g["id"],
                 "escalation_id": 1, "message_id": 1, "skill_id": 1,
                 "watch_id": 1, "credential_id": 1, "session_id": "s1"}

    def synth(name, schema):
        args = {}
        props = schema.get("properties", {})
        for key in schema.get("required", []):
            pdef = props.get(key, {})
            if key in known_ids:
                args[key] = known_ids[key]
            elif pdef.get("enum"):
                args[key] = pdef["enum"][0]
            elif pdef.get("type") == "integer":
                args[key] = 1
            elif pdef.get("type") == "number":
                args[key] = 1.0
            elif pdef.get("type") == "boolean":
                args[key] = False
            elif pdef.get("type") == "array":
                args[key] = []
            elif pdef.get("type") == "object":
                args[key] = {}
            else:
                args[key] = "smoke"
        return args

    tools = _all_tools(mcp)
    assert len(tools) > 150
    failures = []
    for i, t in enumerate(tools):
        req = {"jsonrpc": "2.0", "id": 1000 + i, "method": "tools/call",
               "params": {"name": t["name"],
                          "arguments": synth(t["name"], t["inputSchema"])}}
        try:
            resp = mcp.handle(req)
        except Exception as e:  # handler crashed through the dispatcher
            failures.append((t["name"], f"raised {e!r}"))
            continue
        if resp is None or ("result" not in resp and "error" not in resp):
            failures.append((t["name"], f"bad response {resp!r}"))
    assert not failures, failures


def test_every_tool_survives_dangling_ids(mcp):
    """Second sweep: every tool called with ids that don't exist must return
    a structured response (ok-with-empty or error payload), never crash the
    dispatcher (missing-resource robustness, mirrors the route smoke)."""
    def synth(schema):
        args = {}
        props = schema.get("properties", {})
        for key in schema.get("required", []):
            pdef = props.get(key, {})
            if pdef.get("enum"):
                args[key] = pdef["enum"][0]
            elif pdef.get("type") == "integer":
                args[key] = 999_999          # dangling id
            elif pdef.get("type") == "number":
                args[key] = 999_999.0
            elif pdef.get("type") == "boolean":
                args[key] = True
            elif pdef.get("type") == "array":
                args[key] = []
            elif pdef.get("type") == "object":
                args[key] = {}
            else:
                args[key] = "no-such-thing"
        return args

    failures = []
    for i, t in enumerate(_all_tools(mcp)):
        req = {"jsonrpc": "2.0", "id": 2000 + i, "method": "tools/call",
               "params": {"name": t["name"],
                          "arguments": synth(t["inputSchema"])}}
        try:
            resp = mcp.handle(req)
        except Exception as e:
            failures.append((t["name"], f"raised {e!r}"))
            continue
        if resp is None or ("result" not in resp and "error" not in resp):
            failures.append((t["name"], f"bad response {resp!r}"))
    assert not failures, failures
