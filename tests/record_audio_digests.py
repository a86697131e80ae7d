"""Records tests/golden/audio_digests.json, the fixture of test_audio_digests_gpu.py::test_audio_bits_equal_the_recorded_launches (needs the GPU).

Run it against a library built from the commit whose results are to be kept -- the PARENT of a change that must not alter a bit, never the
changed code itself:

    EFTS_LIB=/path/to/parent/libefts_hip.so python tests/record_audio_digests.py <commit> [output file]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

if __name__ == "__main__":
    import test_audio_digests_gpu as T
    from kernel_check import load_lib

    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else T.DIGESTS
    digests = T.audio_digests(load_lib())
    with open(path, "w") as f:
        json.dump({"recorded_from": commit, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(digests)} launches of {commit} into {path}")
