#!/usr/bin/env python3
"""Record the wire transcript of the UNMODIFIED reference client -> tests/golden/wire_transcript_<scenario>.json.gz.

Needs a checkout of the reference (it is not part of this repository), given as the one argument:

    python tests/golden/gen_wire_transcript.py <reference checkout>

For each of HarfangEnv / HarfangSerpentineEnv / HarfangCircularEnv the reference's own client and wrapper
(hirl/environments/dogfight_client.py + socket_lib.py + HarfangEnv_GYM.py) drive the wire server
(hirl4ucav_amd/environments/wire.py over the CPU oracle simulator) through the closed-loop golden actions
(env_closedloop_<scenario>.npz), and the observations, rewards, done and success flags the wrapper returns are checked
against that golden, as tests/test_wire_cpu.py once did live.  What is written is what crossed the socket: every message
the server received, in order, and for each answered command the reply it sent.  tests/test_wire_cpu.py replays the
messages against the server and requires the same replies, byte for byte — so the fixture holds no code of the
reference, only the data its client wrote and read.
"""
import gzip
import json
import os
import socket
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

CASES = [("HarfangEnv", "straight_line"), ("HarfangSerpentineEnv", "serpentine"), ("HarfangCircularEnv", "circular")]
STEPS = 150  # the closed-loop golden's first 150 steps: ~11 messages each


class _Box:  # the reference imports gym only for spaces.Box(...).sample (HarfangEnv_GYM.py:3,14)
    def __init__(self, low, high, dtype=np.float64):
        self.low, self.high, self.dtype = np.asarray(low), np.asarray(high), dtype

    def sample(self):
        return np.random.uniform(self.low, self.high).astype(self.dtype)


def load_reference(ref):
    gym = types.ModuleType("gym")
    gym.spaces = types.ModuleType("gym.spaces")
    gym.spaces.Box = _Box
    sys.modules["gym"], sys.modules["gym.spaces"] = gym, gym.spaces
    socket.gethostbyname = lambda h: "127.0.0.1"  # socket_lib.py:5-6 resolves the container's hostname at import
    for m in [k for k in sys.modules if k == "hirl" or k.startswith("hirl.")]:  # this repository's alias package has the same name
        del sys.modules[m]
    sys.path.insert(0, ref)
    import hirl.environments.dogfight_client as df
    import hirl.environments.HarfangEnv_GYM as ref_env

    assert os.path.dirname(df.__file__).startswith(os.path.abspath(ref)), df.__file__
    return df, ref_env


def record(df, ref_env, cls, tag):
    from hirl4ucav_amd.environments import wire
    from tests._wire_backend import OracleSimBackend

    class Recorder(wire.WireServer):
        def __init__(self, backend):
            super().__init__(backend)
            self.log = []

        def handle(self, command, args):
            reply = super().handle(command, args)
            entry = {"command": command, "args": args}
            if command in wire.ANSWERED:
                entry["reply"] = reply
            self.log.append(entry)
            return reply

    g = np.load(os.path.join(HERE, f"env_closedloop_{tag}.npz"))
    srv = Recorder(OracleSimBackend()).start()
    try:
        df.connect("127.0.0.1", srv.port)
        df.disable_log(); df.set_renderless_mode(True); df.set_client_update_mode(True)   # train_all.py:149-152
        env = getattr(ref_env, cls)()
        obs = env.reset()
        np.testing.assert_array_equal(np.asarray(obs, np.float64), g["obs0"])
        for t in range(STEPS):
            obs, r, d, _, s = env.step(g["actions"][t])
            np.testing.assert_array_equal(np.asarray(obs, np.float64), g["obs"][t], err_msg=f"obs, step {t}")
            assert float(r) == g["reward"][t] and bool(d) == bool(g["done"][t]) and int(s) == int(g["success"][t]), t
        df.disconnect()
    finally:
        srv.close()
    assert len(srv.log) == srv.messages > 10 * STEPS
    return {"class": cls, "scenario": tag, "steps": STEPS, "messages": srv.log}


def main(argv):
    if len(argv) != 1 or not os.path.isdir(os.path.join(argv[0], "hirl", "environments")):
        raise SystemExit(__doc__)
    df, ref_env = load_reference(argv[0])
    for cls, tag in CASES:
        rec = record(df, ref_env, cls, tag)
        path = os.path.join(HERE, f"wire_transcript_{tag}.json.gz")
        with gzip.GzipFile(path, "wb", mtime=0) as f:  # mtime 0: the same transcript gives the same bytes
            f.write(json.dumps(rec, separators=(",", ":")).encode())
        print(f"{path}: {len(rec['messages'])} messages, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
