"""Child process of tests/test_gpu_score.py: scores ids on a GGUF under the environment the parent set (knobs the library
reads once per process) and prints {"logprobs", "argmax"} as one JSON line.  argv: gguf path, JSON ids, JSON targets."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanollama_amd import gguf, model  # noqa: E402

if __name__ == "__main__":
    dev = model.load_llama_model(gguf.load_gguf(sys.argv[1]))
    lp, am = dev.score(json.loads(sys.argv[2]), json.loads(sys.argv[3]))
    dev.close()
    print(json.dumps({"logprobs": [float(v) for v in lp], "argmax": [int(v) for v in am]}))
