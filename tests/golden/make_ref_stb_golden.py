"""Records tests/golden/ref_stb_digests.json: for every file the decoder tests hold against the reference's stb build (oracle/_ref), the digest of
what that build returned for it, or that it refused it (tests/stb_reference.py).  Runs those tests with the live oracle/_ref and the recorder on.
Run where oracle/_ref is built (make -C oracle ref needs the reference checkout); the fixture then pins the decoders where it is not."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ora  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_stb_digests.json")
TESTS = ["tests/test_jpeg.py", "tests/test_hdr.py", "tests/test_misc_images.py"]

assert ora.have_ref_stb(), "oracle/_ref is not built: make -C oracle ref"
if os.path.exists(OUT):
    os.remove(OUT)
subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "not gpu", *TESTS], cwd=ROOT,
                      env=dict(os.environ, PTC_RECORD_REF_STB=OUT))
print(OUT, os.path.getsize(OUT), "bytes")
