"""Records tests/golden/vocoder_digests.json, the fixture of tests/test_vocoder_digests_gpu.py (needs the GPU).

Run it in a checkout of the commit whose results are to be kept, with that checkout's library built -- the PARENT of a change that must
not alter a bit, never the changed code itself.  It touches only the generator's public surface (see test_vocoder_digests_gpu.py), so this
file and that one can be copied into an older checkout as they are:

    python tests/record_vocoder_digests.py <commit> [output file]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

if __name__ == "__main__":
    import test_vocoder_digests_gpu as T

    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else T.DIGESTS
    digests = T.vocoder_digests()
    with open(path, "w") as f:
        json.dump({"recorded_from": commit, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(digests)} forward passes of {commit} into {path}")
