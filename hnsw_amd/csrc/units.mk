# The units of beam_units.hip and walks_units.hip: one object per unit, each
# compiled from the one source with -DMH_UNIT=<unit> (the sources say what a
# unit holds).  Included by the library's Makefile and by tools/Makefile.beam.
BEAM_UNITS := beam_a beam_b beam_c beam_d beam_x2a beam_x2b beam_x4a beam_x4b \
              beam_w1a beam_w1b beam_w2a beam_w2b beam_w4a beam_w4b beam_fa beam_fb beam_desc
WALKS_UNITS := walks_a walks_b walks_c walks_d
