for c in 32 64 96 128 192 256; do echo "chunk $c"; ANX_SCAN_CHUNK_FUSED=$c bash tools/quick_ab.sh tree 2>&1 | tail -1; done
# the first reservation of a wave (doubled up to the chunk; 128 = flat reservations at the default chunk)
for f in 32 64 128; do echo "first $f"; ANX_SCAN_CHUNK_FIRST=$f bash tools/quick_ab.sh tree 2>&1 | tail -1; done
