"""Inputs and oracle references of the ragged-corpus tests (tests/test_gpu_crops_ragged*.py): files of very different length
per geometry, as corpus_testlib.Files; a test lays them out with corpus_testlib.Corpus (None: a file nobody crops).  CPU only."""
import functools
from corpus_testlib import oracle_file

FILE_BLOCKS = (1, 2, 7, 12, 40)
# geometry -> (VBR quality, synth_pcm stream id of the 40-block file: the stream of seek_testlib.ORACLE_CASES; the shorter files
# take the ids behind it).  Stereo 2048 runs the specialised synthesis, the other two the general one.
GEOMS = {(2048, 2): (50.0, 3), (1024, 1): (20.0, 11), (2048, 3): (60.0, 3)}


@functools.lru_cache(maxsize=None)
def file_refs(geom):
    bs, ch = geom
    q, sid = GEOMS[geom]
    out = []
    for i, K in enumerate(FILE_BLOCKS):
        out.append(oracle_file(bs, ch, q, sid) if K == 40 else oracle_file(bs, ch, q, sid + 1 + i, 11, K))
        assert (out[-1].bits > 0).all()
    return out
