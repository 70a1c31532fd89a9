"""The wire-protocol server (hirl4ucav_amd/environments/wire.py) on CPU: framing and command handling against a raw client, and the
transcripts of the UNMODIFIED reference client and wrapper (hirl/environments/dogfight_client.py + socket_lib.py + HarfangEnv_GYM.py)
driving the server over loopback TCP through the closed-loop golden traces (which were recorded from the same reference classes over an
in-process fake of dogfight_client), replayed against the server (tests/golden/wire_transcript_*.json.gz)."""
import gzip
import json
import os

import numpy as np
import pytest

from hirl4ucav_amd.environments import wire
from tests._wire_backend import ALLY, OPPO, OracleSimBackend, RawClient


def test_framing_and_commands_with_a_raw_client():
    srv = wire.WireServer(OracleSimBackend()).start()
    try:
        c = RawClient(srv.port)
        assert c.ask("GET_PLANESLIST")[0] == ALLY and c.ask("GET_PLANESLIST")[3] == OPPO
        for cmd in ("DISABLE_LOG", "RETRACT_GEAR"):
            c.send(cmd, plane_id=ALLY)                                  # unanswered commands must not produce a reply
        c.send("SET_RENDERLESS_MODE", flag=True)
        # the reset sequence of HarfangEnv._reset_machine / _reset_missile (HarfangEnv_GYM.py:171-188)
        c.send("RESET_MACHINE", machine_id=OPPO); c.send("RESET_MACHINE", machine_id=ALLY)
        c.send("SET_HEALTH", machine_id=OPPO, health_level=0.2)
        c.send("RESET_MACHINE_MATRIX", machine_id=OPPO, position=[0, 4200, 0], rotation=[0, 0, 0])
        c.send("RESET_MACHINE_MATRIX", machine_id=ALLY, position=[10, 3500, -4000], rotation=[0, 0, 0])
        c.send("SET_PLANE_THRUST", plane_id=ALLY, thrust_level=1); c.send("SET_PLANE_THRUST", plane_id=OPPO, thrust_level=0.6)
        c.send("SET_PLANE_LINEAR_SPEED", plane_id=ALLY, linear_speed=300); c.send("SET_PLANE_LINEAR_SPEED", plane_id=OPPO, linear_speed=200)
        c.send("REARM_MACHINE", machine_id=ALLY)
        st = c.ask("GET_PLANE_STATE", plane_id=ALLY)
        assert st["position"] == [10.0, 3500.0, -4000.0] and st["Euler_angles"] == [0.0, 0.0, 0.0] and st["target_locked"] is False
        assert abs(st["target_angle"] - np.degrees(np.arccos(4000 / np.sqrt(10 ** 2 + 700 ** 2 + 4000 ** 2)))) < 1e-3
        assert c.ask("GET_HEALTH", machine_id=OPPO) == {"health_level": pytest.approx(0.2)}
        assert c.ask("GET_MISSILESDEVICE_SLOTS_STATE", machine_id=ALLY) == {"missiles_slots": [True]}
        z0 = st["position"][2]
        c.send("SET_PLANE_PITCH", plane_id=ALLY, pitch_level=-0.3); c.send("FIRE_MISSILE", machine_id=ALLY, slot_id=0)
        c.send("UPDATE_SCENE")
        st = c.ask("GET_PLANE_STATE", plane_id=ALLY)
        assert 4.5 < st["position"][2] - z0 < 5.5 and st["user_pitch_level"] == -0.3      # 300 m/s for 1/60 s
        assert c.ask("GET_MISSILESDEVICE_SLOTS_STATE", machine_id=ALLY) == {"missiles_slots": [False]}
        assert c.ask("IS_IA_ACTIVATED", machine_id=ALLY) == {}                              # answered, even if nothing to say
        c.close()
    finally:
        srv.close()


@pytest.mark.parametrize("cls,tag", [("HarfangEnv", "straight_line"), ("HarfangSerpentineEnv", "serpentine"), ("HarfangCircularEnv", "circular")])
def test_unmodified_reference_client_drives_the_server(cls, tag, golden_dir):
    """Replays what the reference's own client and wrapper sent over loopback TCP while they stepped through the closed-loop golden actions
    (tests/golden/gen_wire_transcript.py: there their observations, rewards and flags were checked against env_closedloop_<tag>.npz) and
    requires the server to answer every answered command with the bytes that client read then: same replies -> same wrapper results."""
    with gzip.open(os.path.join(golden_dir, f"wire_transcript_{tag}.json.gz"), "rb") as f:
        rec = json.loads(f.read().decode())
    assert rec["class"] == cls and rec["scenario"] == tag
    msgs, n = rec["messages"], rec["steps"]
    assert sum(m["command"] == "UPDATE_SCENE" for m in msgs) >= n
    srv = wire.WireServer(OracleSimBackend()).start()
    try:
        c = RawClient(srv.port)
        for k, m in enumerate(msgs):
            body = json.dumps({"command": m["command"], "args": m["args"]}).encode()
            c.s.sendall(len(body).to_bytes(4, "big") + body)
            if "reply" in m:
                got = c._exact(int.from_bytes(c._exact(4), "big")).decode()
                assert got == json.dumps(m["reply"]), (k, m["command"], m["args"])
        c.close()
        assert srv.messages == len(msgs) > 10 * n
    finally:
        srv.close()


def test_server_survives_malformed_messages():
    """an oversize length prefix, broken JSON, a missing 'command' key or an unknown machine id must close that
    connection only; the server keeps serving the next client."""
    import json
    import socket
    import time

    from hirl4ucav_amd.environments import wire
    from tests._wire_backend import OracleSimBackend, RawClient

    srv = wire.WireServer(OracleSimBackend(), "127.0.0.1", 0).start()
    try:
        for payload in (b"\xff\xff\xff\xff", (5).to_bytes(4, "big") + b"{nope",
                        (lambda b: len(b).to_bytes(4, "big") + b)(json.dumps({"args": {}}).encode()),
                        (lambda b: len(b).to_bytes(4, "big") + b)(json.dumps({"command": "GET_PLANE_STATE", "args": {"plane_id": "intruder"}}).encode())):
            s = socket.create_connection(("127.0.0.1", srv.port))
            s.sendall(payload)
            s.settimeout(5)
            assert s.recv(16) == b""  # the server closed this connection
            s.close()
        time.sleep(0.05)
        c = RawClient(srv.port)  # ... and still answers a well-formed client
        assert c.ask("GET_HEALTH", machine_id="ennemy_2")["health_level"] > 0
        c.close()
    finally:
        srv.close()
