"""The stored fixtures of the data / finetuning / tokenizer tests (``tests/golden/transformer_files``: the small
datasets, index caches and the LLaMA-2 tokenizer of the reference's ``tests/transformer/files``).

``FILES`` is a private, writable copy made once per process: datasets write their index caches next to the data
they open, and the tokenizer is stored gzip-compressed (the plain JSON is over the size limit for a committed
file).  The committed files are never written to."""
import atexit
import gzip
import os
import shutil
import tempfile
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden"

_tmp = Path(tempfile.mkdtemp(prefix="scaling_amd_golden_"))
_owner = os.getpid()


@atexit.register
def _cleanup() -> None:
    if os.getpid() == _owner:  # not from a forked child
        shutil.rmtree(_tmp, ignore_errors=True)



FILES = _tmp / "files"
shutil.copytree(GOLDEN / "transformer_files", FILES, ignore=shutil.ignore_patterns("*.gz"))
TOKENIZER = FILES / "llama2-tokenizer.json"
with gzip.open(GOLDEN / "transformer_files" / "llama2-tokenizer.json.gz", "rb") as _src, open(TOKENIZER, "wb") as _dst:
    shutil.copyfileobj(_src, _dst)
