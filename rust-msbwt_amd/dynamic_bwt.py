"""Construction from read files: the counterpart of the reference's `DynamicBWT::create_from_fastx`
(src/dynamic_bwt.rs:453-473) and of its `msbwt2-build` binary, with the sort on the MI355X (csrc/reads_build.hip)."""
import gzip

import numpy as np

from .rle_bwt import RleBWT

# needletail's normalize(false) followed by convert_stoi (string_util.rs:15-32): A/a C/c G/g T/t keep their letter, U/u is T,
# blanks and line ends vanish, every other byte ('-', '.', IUPAC codes, '$') ends as N
_CODES = bytearray([4]) * 256
for _letters, _code in ((b"Aa", 1), (b"Cc", 2), (b"Gg", 3), (b"TtUu", 5)):
    for _b in _letters:
        _CODES[_b] = _code
_CODES = bytes(_CODES)
_BLANKS = b" \t\r\n"


def sequence_codes(seq):
    """One record's sequence bytes -> symbol codes (np.uint8[])."""
    return np.frombuffer(bytes(seq).translate(_CODES, _BLANKS), dtype=np.uint8)


def _open(filename):
    with open(filename, "rb") as f:
        magic = f.read(2)
    return gzip.open(filename, "rb") if magic == b"\x1f\x8b" else open(filename, "rb")


def read_fastx(filename):
    """Yields (name, sequence bytes as written) for every record of a FASTA (sequences may span lines) or four-line FASTQ
    file, plain or gzipped."""
    with _open(filename) as f:
        line = f.readline()
        while line and not line.strip():
            line = f.readline()
        if not line:
            return
        if line[:1] == b">":
            name, parts = line[1:].strip(), []
            for line in f:
                if line[:1] == b">":
                    yield name, b"".join(parts)
                    name, parts = line[1:].strip(), []
                else:
                    parts.append(line.rstrip(b"\r\n"))
            yield name, b"".join(parts)
        elif line[:1] == b"@":
            while line:
                if line[:1] != b"@":
                    raise ValueError("%s: a FASTQ record must start with '@', found %r" % (filename, line[:20]))
                seq, plus, qual = f.readline(), f.readline(), f.readline()
                if plus[:1] != b"+" or not qual:
                    raise ValueError("%s: truncated FASTQ record %r" % (filename, line.strip()[:40]))
                yield line[1:].strip(), seq.rstrip(b"\r\n")
                line = f.readline()
                while line and not line.strip():
                    line = f.readline()
        else:
            raise ValueError("%s: neither FASTA ('>') nor FASTQ ('@')" % filename)


def reads_from_fastx(filenames):
    """Every sequence of the files, in file order, as symbol-code arrays."""
    if isinstance(filenames, (str, bytes)) or hasattr(filenames, "__fspath__"):
        filenames = [filenames]
    return [sequence_codes(seq) for fn in filenames for _, seq in read_fastx(fn)]


def create_from_fastx(filenames, sorted=True, device=None):
    """An RleBWT holding the multi-string BWT of the files' reads; its `rle` attribute keeps the RLE bytes, for
    bwt_converter.save_bwt_numpy (what msbwt2-build writes).  Only the sorted form exists: the reference's own binary never asks
    for the other (msbwt2-build.rs:45-47)."""
    if not sorted:
        raise NotImplementedError("only the sorted multi-string BWT is built")
    bwt = RleBWT(device=-1 if device is None else device)
    bwt.rle = bwt.build_from_reads(reads_from_fastx(filenames))
    bwt.load_vector(bwt.rle)
    return bwt
